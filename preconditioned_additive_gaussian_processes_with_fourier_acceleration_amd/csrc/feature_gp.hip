// feature_gp.hip -- the exact GP loss, its gradient, the solve and the variance matrix in feature space.
//
// With 1-D windows the operator is A = f^2 (Z W Z^T + mu I) (model_variance.hip's header): Z holds 33
// trigonometric features per window of the window's quantised coordinate and W is diagonal.  A handle's centres and
// scales are fixed at its first setup, so only W depends on the hyperparameters: G = Z^T Z, b = Z^T y and y^T y are
// formed once per data set (window_moments) and everything after is R x R work, R = 33 nw.  With
//   B = mu I + W G,  v = B^{-1} (w o b),  u = (b - G v) / mu = Z^T M^{-1} y,  M = Z W Z^T + mu I
//   q = (y^T y - b^T v) / mu = y^T M^{-1} y,   |M^{-1} y|^2 = (y^T y - 2 v^T b + v^T G v) / mu^2
//   log det A = n log f^2 + (n - R) log mu + log |det B|                       (Sylvester; n < R too)
// the reference's loss (gp_loss.c:224-283) is  1/2 (q / (f^2 n) + log det A / n + log 2 pi)  and its gradient
// 1/2 (-L1_i + L2_i) dt_i with
//   n L1 = 2 q / f^3,  u^T (w' o u) / f^2,  |M^{-1} y|^2 / f^2            (f, l, mu)
//   n L2 = 2 n / f,    tr(B^{-1} diag(w') G),  (n - R) / mu + tr(B^{-1})
// w' = dW/dl (feature_weights_grad).  alpha = (y - Z v) / (f^2 mu) solves A alpha = y, S = mu B^{-1} W symmetrised
// is the matrix of Nfft4GPAmdModelFitVariance, and the posterior mean at a point with features phi is phi^T (w o u).
// W has negative entries, so B is factored by LU; the loss uses log |det B| and the sign of det B is only reported.
// Internally the slots are padded as in model_variance.hip (36 per window, windows to a multiple of 4): a padded slot
// has zero weight and zero features, B keeps mu on its diagonal there, and (R_p - R) log mu leaves the factor's
// log-determinant again.
// The leave-one-out loss, gradient and per-point predictions (k_fgp_loo, further down) need diag(A^{-1}): one
// quadratic form per training point with an R x R matrix, on the walk of k_model_std.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.h"
#include "quad_walk.hpp"

namespace nfft4gp_amd {
namespace {

constexpr int kFaThreads = 256;
constexpr int kFaPts = 4;  // points per thread, strided by the workgroup (coalesced columns, 4 independent chains)
constexpr int kFsThreads = 256;

struct FeatureGp {
   int n = 0, nw = 0, d = 0, kernel = 0, Rp = 0, R = 0;
   std::vector<double> scale;   // host copy (the weights are formed on the host: 33 nw values)
   double* d_centre = nullptr;  // [nw]
   double* d_scale = nullptr;   // [nw]
   int* d_feature = nullptr;    // [nw]
   double* d_G = nullptr;       // [R_p][R_p] Z^T Z
   double* d_by = nullptr;      // [R_p] Z^T y, then y^T y
   double yy = 0.0;
   int transform = 0;
   bool has_mask = false;
   int mask[3] = {1, 1, 1};
   // the last evaluation
   int det_sign = 0;
   double logabsdet = 0.0;
   bool factored = false;  // d_Binv and d_vec hold the quantities of (fl, fmu)
   double fl = 0.0, fmu = 0.0;
   double sc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // b^T v, v^T G v, u^T (w' o u), tr B^{-1}, tr(B^{-1} diag(w') G)
   // scratch of an evaluation
   double* d_B = nullptr;     // [R_p][R_p] mu I + W G, then its factors
   double* d_Binv = nullptr;  // [R_p][R_p + 1] B^{-1}, then v = B^{-1} (w o b): one solve, R_p + 1 right-hand sides
   int* d_piv = nullptr;      // the factorisation's row interchanges (further right-hand sides: lu_resolve_dev)
   double* d_vec = nullptr;   // [7][R_p]: w, w', v, G v, w o u, column sums of the trace, 8 scalars
   BlockCounts counts;        // per-workgroup counts of outside points
   // leave-one-out (Nfft4GPAmdFeatureGpLooBind): the data, borrowed device arrays or copies the object owns
   const double* loo_X = nullptr;
   const double* loo_y = nullptr;
   long long loo_ld = 0;
   double *loo_Xown = nullptr, *loo_yown = nullptr;
   double* d_looQ = nullptr;     // [3][R_p][R_p] sym(B^{-1} W), Q_l, Q_G, then two R_p x R_p scratch matrices
   double* d_loocoef = nullptr;  // [3][R_p] v, c_l, c_mu
   double* d_loopart = nullptr;  // [blocks + 1][kLooSums] per-workgroup sums; the last row their sum
   size_t loopart_cap = 0;
   long long loo_nonpositive = 0;  // points with m_i <= 0 at the last leave-one-out evaluation
};
enum { kVw = 0, kVdw, kVv, kVgv, kVwu, kVpart, kVscal };
// a workgroup's sums: the loss terms, the three gradient terms, the points with m_i <= 0, the points outside the domain
constexpr int kLooSums = 6;

void loo_unbind(FeatureGp* F)
{
   for (double* p : {F->loo_Xown, F->loo_yown})
      if (p) (void)hipFree(p);
   F->loo_Xown = F->loo_yown = nullptr;
   F->loo_X = F->loo_y = nullptr;
   F->loo_ld = 0;
}

void fgp_free(FeatureGp* F)
{
   if (!F) return;
   loo_unbind(F);
   for (void* p : {(void*)F->d_centre, (void*)F->d_scale, (void*)F->d_feature, (void*)F->d_G, (void*)F->d_by,
                   (void*)F->d_B, (void*)F->d_Binv, (void*)F->d_piv, (void*)F->d_vec,
                   (void*)F->d_looQ, (void*)F->d_loocoef, (void*)F->d_loopart})
      if (p) (void)hipFree(p);
   delete F;
}

// B = mu I + W G and the right-hand sides [I | w o b] of its solve (rhs: column R_p of Binv)
__global__ void k_fgp_system(const double* __restrict__ G, const double* __restrict__ w, const double* __restrict__ b,
                             int Rp, double mu, double* __restrict__ B, double* __restrict__ Binv,
                             double* __restrict__ rhs)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= Rp) return;
   const size_t e = i + (size_t)j * Rp;
   B[e] = w[i] * G[e] + (i == j ? mu : 0.0);
   Binv[e] = (i == j) ? 1.0 : 0.0;
   if (j == 0) rhs[i] = w[i] * b[i];
}

__global__ void k_fgp_hadamard(const double* __restrict__ w, const double* __restrict__ b, int Rp,
                               double* __restrict__ out)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < Rp) out[i] = w[i] * b[i];
}

// the workgroup's sum of v over its threads in a fixed tree; every thread returns it
__device__ inline double fgp_block_sum(double v, double* s_red)
{
   const int t = threadIdx.x;
   __syncthreads();  // the previous sum's readers are done
   s_red[t] = v;
   __syncthreads();
   for (int h = kFsThreads / 2; h > 0; h >>= 1) {
      if (t < h) s_red[t] += s_red[t + h];
      __syncthreads();
   }
   return s_red[0];
}

// part[j] = w'_j sum_i Binv(i, j) G(i, j): column j's share of tr(B^{-1} diag(w') G) (G is symmetric); one workgroup
// per column, a thread adds its rows in order
__global__ __launch_bounds__(kFsThreads) void k_fgp_trace_cols(const double* __restrict__ Binv,
                                                               const double* __restrict__ G,
                                                               const double* __restrict__ dw, int Rp,
                                                               double* __restrict__ part)
{
   __shared__ double s_red[kFsThreads];
   const int j = blockIdx.x;
   const double* bc = Binv + (size_t)j * Rp;
   const double* gc = G + (size_t)j * Rp;
   double acc = 0.0;
   for (int i = threadIdx.x; i < Rp; i += kFsThreads) acc = fma(bc[i], gc[i], acc);
   const double t = fgp_block_sum(acc, s_red);
   if (threadIdx.x == 0) part[j] = dw[j] * t;
}

// One workgroup: wu = w o u with u = (b - G v) / mu, and the five scalars of an evaluation, each one fixed-order
// reduction over the slots: out = b^T v, v^T G v, u^T (w' o u), tr B^{-1} over the real slots, sum of part
__global__ __launch_bounds__(kFsThreads) void k_fgp_scalars(const double* __restrict__ b, const double* __restrict__ w,
                                                            const double* __restrict__ dw,
                                                            const double* __restrict__ v, const double* __restrict__ Gv,
                                                            const double* __restrict__ Binv,
                                                            const double* __restrict__ part, int Rp, int nw, double mu,
                                                            double* __restrict__ wu, double* __restrict__ out)
{
   __shared__ double s_red[kFsThreads];
   double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
   for (int i = threadIdx.x; i < Rp; i += kFsThreads) {
      const double u = (b[i] - Gv[i]) / mu;
      wu[i] = w[i] * u;
      a[0] = fma(b[i], v[i], a[0]);
      a[1] = fma(v[i], Gv[i], a[1]);
      a[2] = fma(dw[i] * u, u, a[2]);
      const bool real = (i % kMvPad) < kMvFeat && (i / kMvPad) < nw;  // a padded slot's 1 / mu is not part of tr B^{-1}
      if (real) a[3] += Binv[i + (size_t)i * Rp];
      a[4] += part[i];
   }
   for (int k = 0; k < 5; k++) {
      const double t = fgp_block_sum(a[k], s_red);
      if (threadIdx.x == 0) out[k] = t;
   }
}

// S (R x R row-major, unpadded) = mu B^{-1} W symmetrised
__global__ void k_fgp_variance(const double* __restrict__ Binv, const double* __restrict__ w, int Rp, int R, double mu,
                               double* __restrict__ S)
{
   const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
   if (j >= R) return;
   const int ip = mv_slot(i), jp = mv_slot(j);
   S[(size_t)i * R + j] = 0.5 * (mu * Binv[ip + (size_t)jp * Rp] * w[jp] + mu * Binv[jp + (size_t)ip * Rp] * w[ip]);
}

// out = a y + c (Z coef) over n points (y may be NULL: out = c (Z coef)).  One thread owns kFaPts points, strided by
// the workgroup as in k_model_predict; the R_p coefficients sit in LDS (<= 36.9 KB at 128 windows, 9.2 KB at 32: 8
// workgroups of 4 waves fill a CU's wave slots at 74 KB of its 160 KB) and every lane of a wave reads the same
// address at the same time: a broadcast, no bank conflict.  Per (point, window): one coalesced coordinate load,
// mv_angle, 16 mv_rotate steps and 33 FMAs -- about 170 flops per 8 bytes read, so the kernel is bound by the vector
// fp64 rate and the 4 points per thread are its independent dependency chains.  A point's windows are added in
// the order c = 0 .. nw - 1 by its own thread: no atomics, the same bits however the points are batched and
// wherever the arrays came from.  A point outside a window's domain is NaN and counted (cnt_out may be NULL).
__global__ __launch_bounds__(kFaThreads) void k_fgp_apply(const double* __restrict__ coef, int Rp,
                                                          const double* __restrict__ centre,
                                                          const double* __restrict__ scale,
                                                          const int* __restrict__ feature, int nw,
                                                          const double* __restrict__ X, long long ldim, int n,
                                                          const double* __restrict__ y, double a, double c,
                                                          double* __restrict__ out, unsigned int* __restrict__ cnt_out)
{
   extern __shared__ double f_coef[];
   const int tid = threadIdx.x;
   for (int i = tid; i < Rp; i += kFaThreads) f_coef[i] = coef[i];
   __syncthreads();
   const long long base = (long long)blockIdx.x * (kFaThreads * kFaPts) + tid;
   double acc[kFaPts];
   bool outside[kFaPts];
#pragma unroll
   for (int p = 0; p < kFaPts; p++) {
      acc[p] = 0.0;
      outside[p] = false;
   }
   for (int w = 0; w < nw; w++) {
      const double ctr = centre[w], sc = scale[w];
      const double* col = X + (size_t)feature[w] * (size_t)ldim;
      const double* cf = f_coef + w * kMvPad;
      double c1[kFaPts], s1[kFaPts], ck[kFaPts], sk[kFaPts];
#pragma unroll
      for (int p = 0; p < kFaPts; p++) {
         const long long i = base + (long long)p * kFaThreads;
         const double xv = (i < n) ? col[i] : ctr;
         outside[p] = !mv_angle(xv, ctr, sc, c1[p], s1[p]) || outside[p];
         acc[p] = fma(cf[0], 1.0, acc[p]);  // k = 0: cos 0
         ck[p] = c1[p];
         sk[p] = s1[p];
      }
#pragma unroll
      for (int k = 1; k <= 16; k++) {
         const double cc = cf[k], cs = cf[16 + k];
#pragma unroll
         for (int p = 0; p < kFaPts; p++) {
            acc[p] = fma(cc, ck[p], acc[p]);
            acc[p] = fma(cs, sk[p], acc[p]);
            if (k < 16) mv_rotate(ck[p], sk[p], c1[p], s1[p]);
         }
      }
   }
#pragma unroll
   for (int p = 0; p < kFaPts; p++) {
      const long long i = base + (long long)p * kFaThreads;
      const bool live = i < n;
      if (live) {
         const double zc = c * acc[p];
         out[i] = outside[p] ? __builtin_nan("") : (y ? fma(a, y[i], zc) : zc);
      }
      outside[p] = live && outside[p];
   }
   block_count_outside<kFaThreads>(outside, cnt_out);
}

WindowMap window_map(const FeatureGp* F) { return WindowMap{F->nw, F->d, F->d_centre, F->d_scale, F->d_feature}; }

// B^{-1}, v, G v, w o u and the scalars at (l, mu); kept until other hyperparameters are asked for.  0, -1 (bad
// hyperparameters, a zero pivot, a HIP error)
int fgp_factor(FeatureGp* F, double l, double mu)
{
   if (!(mu > 0.0) || !(l > 0.0) || !std::isfinite(mu) || !std::isfinite(l)) return -1;
   if (F->factored && F->fl == l && F->fmu == mu) return 0;
   F->factored = false;
   F->det_sign = 0;
   hipStream_t s = current_stream();
   const int Rp = F->Rp, nw = F->nw;
   const size_t rr = (size_t)Rp * Rp;
   if (!F->d_B) {
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_B, sizeof(double) * rr));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_Binv, sizeof(double) * (rr + Rp)));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_piv, sizeof(int) * (size_t)Rp));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_vec, sizeof(double) * 7 * (size_t)Rp));
   }
   double* V = F->d_vec;
   auto vec = [&](int which) { return V + (size_t)which * Rp; };
   std::vector<double> w(2 * (size_t)Rp, 0.0);
   for (int c = 0; c < nw; c++) {
      feature_weights(F->kernel, l, F->scale[c], nw, w.data() + (size_t)c * kMvPad);
      feature_weights_grad(F->kernel, l, F->scale[c], nw, w.data() + Rp + (size_t)c * kMvPad);
   }
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(vec(kVw), w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));  // w leaves scope; the copy from pageable memory has been staged
   hipLaunchKernelGGL(k_fgp_system, dim3((Rp + 255) / 256, Rp), dim3(256), 0, s, (const double*)F->d_G,
                      (const double*)vec(kVw), (const double*)F->d_by, Rp, mu, F->d_B, F->d_Binv, F->d_Binv + rr);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   double lad = 0.0;
   int sign = 0;
   // v comes out of the factors' own substitution (backward stable), not from the explicit inverse: alpha's
   // residual would otherwise carry cond(B) / mu
   if (const int info = lu_solve_dev(F->d_B, Rp, F->d_Binv, Rp + 1, s, &lad, &sign, F->d_piv)) {
      if (info > 0) fprintf(stderr, "nfft4gp_amd: feature GP: mu I + W G has a zero pivot in column %d.\n", info);
      return -1;
   }
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(vec(kVv), F->d_Binv + rr, sizeof(double) * Rp, hipMemcpyDeviceToDevice, s));
   if (gemm_f64(false, Rp, 1, Rp, F->d_G, Rp, vec(kVv), Rp, vec(kVgv), Rp, s)) return -1;
   hipLaunchKernelGGL(k_fgp_trace_cols, dim3(Rp), dim3(kFsThreads), 0, s, (const double*)F->d_Binv,
                      (const double*)F->d_G, (const double*)vec(kVdw), Rp, vec(kVpart));
   hipLaunchKernelGGL(k_fgp_scalars, dim3(1), dim3(kFsThreads), 0, s, (const double*)F->d_by, (const double*)vec(kVw),
                      (const double*)vec(kVdw), (const double*)vec(kVv), (const double*)vec(kVgv),
                      (const double*)F->d_Binv, (const double*)vec(kVpart), Rp, nw, mu, vec(kVwu), vec(kVscal));
   NFFT4GP_HIP_CHECK(hipGetLastError());
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(F->sc, vec(kVscal), sizeof(double) * 5, hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   F->logabsdet = lad - (double)(Rp - F->R) * std::log(mu);  // the padded slots' pivots are mu
   F->det_sign = sign;
   F->fl = l;
   F->fmu = mu;
   F->factored = true;
   return 0;
}

// out = a y + c Z coef at the n rows of X (X, y, out: host or device); *n_outside: the rows outside the domain
int fgp_apply(FeatureGp* F, const double* coef, const double* X, int n, long long ldim, const double* y, double a,
              double c, double* out, long long* n_outside)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   const double *dX, *dy = nullptr;
   long long ld, ldy;
   if (stage(sc, X, (size_t)n, (size_t)F->d, (size_t)ldim, &dX, &ld)) return -1;
   if (y && stage(sc, y, (size_t)n, 1, (size_t)n, &dy, &ldy)) return -1;
   double* dout = out;
   const bool odev = is_device_ptr(out);
   if (!odev && sc.alloc(&dout, (size_t)n)) return -1;
   const int per = kFaThreads * kFaPts;
   const size_t nblk = ((size_t)n + per - 1) / per;
   if (F->counts.grow(nblk)) return -1;
   hipLaunchKernelGGL(k_fgp_apply, dim3((unsigned int)nblk), dim3(kFaThreads), sizeof(double) * (size_t)F->Rp, s, coef,
                      F->Rp, (const double*)F->d_centre, (const double*)F->d_scale, (const int*)F->d_feature, F->nw, dX,
                      ld, n, dy, a, c, dout, F->counts.d);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (!odev) NFFT4GP_HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
   return F->counts.read(nblk, s, n_outside);  // synchronises: nothing in flight reads the staging buffers
}

// ---- leave-one-out -------------------------------------------------------------------------------
// With P = B^{-1} W and phi a training point's features: [M^{-1}]_ii = m_i = (1 - phi^T P phi) / mu and
// [M^{-1} y]_i = a_i = (y_i - phi^T v) / mu (Z^T M^{-1} e_i = B^{-T} phi).  The point's leave-one-out mean is
// y_i - a_i / m_i, its variance f^2 / m_i, and the loss 1/(2n) sum_i log(f^2 / |m_i|) + a_i^2 / (f^2 m_i) + log 2 pi.
//   dm_i/dl  = -phi^T Q_l phi,  Q_l = B^{-1} diag(w') B^{-T}        da_i/dl  = -phi^T c_l,  c_l = B^{-1} (w' o u)
//   dm_i/dmu = -(1 - 2 p_i + phi^T Q_G phi) / mu^2,  Q_G = P^T G P   da_i/dmu = -(a_i - phi^T c_mu) / mu,
//   c_mu = B^{-1} (w o u)
// so an evaluation is three symmetric quadratic forms and three linear forms per point.  m_i can be <= 0 (the
// operator is not always definite): log |m_i|, the signed m_i elsewhere, and such points are counted.

// Q0 = the symmetric part of B^{-1} W; T1 = B^{-T}; T2 = diag(w') B^{-T} (all R_p x R_p column-major)
__global__ void k_fgp_loo_mats(const double* __restrict__ Binv, const double* __restrict__ w,
                               const double* __restrict__ dw, int Rp, double* __restrict__ Q0,
                               double* __restrict__ T1, double* __restrict__ T2)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= Rp) return;
   const size_t e = i + (size_t)j * Rp;
   const double bij = Binv[e], bji = Binv[j + (size_t)i * Rp];
   Q0[e] = 0.5 * (bij * w[j] + bji * w[i]);
   T1[e] = bji;
   T2[e] = dw[i] * bji;
}

// T = B^{-1} W
__global__ void k_fgp_loo_scale(const double* __restrict__ Binv, const double* __restrict__ w, int Rp,
                                double* __restrict__ T)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= Rp) return;
   const size_t e = i + (size_t)j * Rp;
   T[e] = Binv[e] * w[j];
}

// Q <- (Q + Q^T) / 2 in place: the thread of (i, j), i < j, writes both entries
__global__ void k_fgp_loo_symmetrise(double* __restrict__ Q, int Rp)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= j) return;
   const size_t e = i + (size_t)j * Rp, et = j + (size_t)i * Rp;
   const double v = 0.5 * (Q[e] + Q[et]);
   Q[e] = v;
   Q[et] = v;
}

// coef = [v | w' o u | w o u], u = (b - G v) / mu: the right-hand sides of c_l and c_mu behind v
__global__ void k_fgp_loo_rhs(const double* __restrict__ b, const double* __restrict__ dw,
                              const double* __restrict__ v, const double* __restrict__ Gv,
                              const double* __restrict__ wu, int Rp, double mu, double* __restrict__ coef)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= Rp) return;
   coef[i] = v[i];
   coef[Rp + i] = dw[i] * ((b[i] - Gv[i]) / mu);
   coef[2 * (size_t)Rp + i] = wu[i];
}

// k_fgp_loo: one pass over the n training points, 128 per workgroup.  The three matrices of Q (sym P, Q_l, Q_G;
// R_p^2 apart) are walked one after another by quad_walk.hpp's walk (k_model_std's: an S tile and its feature panel
// already fill the LDS, so there is no room for three tiles against one panel, and three tiles' accumulators do not
// fit the registers); the first walk's epilogue, which generates every window's features once per point, also dots
// them with v, c_l and c_mu, a quarter of a window per thread.  A point's six sums run in a fixed order that depends
// on neither its place in the batch nor n.  The epilogue forms the point's loss term and three gradient terms
// (before dt and 1 / 2n) and, when asked, its leave-one-out mean and variance; the workgroup's kLooSums sums fold
// over the wave in a fixed butterfly, then over the waves in wave order; sum_parts_dev adds the workgroups in block
// order.  No atomics.  A point outside a window's domain (the wrong X was bound) is counted and the caller refuses:
// mv_angle gives it the angle 0, so nothing is NaN.
__global__ __launch_bounds__(kMsThreads) void k_fgp_loo(const double* __restrict__ Q, int Rp,
                                                        const double* __restrict__ coef,
                                                        const double* __restrict__ centre,
                                                        const double* __restrict__ scale,
                                                        const int* __restrict__ feature, int nw,
                                                        const double* __restrict__ X, long long ldim, int n,
                                                        const double* __restrict__ y, double f, double mu,
                                                        double* __restrict__ mean_out, double* __restrict__ var_out,
                                                        double* __restrict__ part_out)
{
   extern __shared__ double m_smem[];
   __shared__ double s_q[3][kMsPts];
   __shared__ double s_red[kMsThreads / kWave][kLooSums];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int p = tid & (kMsPts - 1), part = tid >> 7;
   const long long ip = (long long)blockIdx.x * kMsPts + p;
   const bool live = ip < n;
   quad_zero_pad(m_smem);
   const QuadPoints P{centre, scale, feature, nw, X, ldim, ip, live};
   double lin[3] = {0.0, 0.0, 0.0};
   for (int m = 0; m < 3; m++) {
      const double psum = quad_walk<3>(Q + (size_t)m * Rp * Rp, Rp, P, m_smem, m == 0, coef, Rp, lin);
      quad_fold(psum, s_q[m]);
   }
   __syncthreads();  // the last walk has left the buffers
   double* s_lin = m_smem;  // [form][part][point]
#pragma unroll
   for (int q = 0; q < 3; q++) s_lin[(q * 4 + part) * kMsPts + p] = lin[q];
   __syncthreads();
   double t[kLooSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
   if (part == 0 && live) {  // waves 0 and 1 own the 128 points from here; the others add exact zeros
      const bool outside = row_outside(centre, scale, feature, nw, X, ldim, ip);
      double l3[3];
#pragma unroll
      for (int q = 0; q < 3; q++) {
         const double* sl = s_lin + q * 4 * kMsPts + p;
         l3[q] = ((sl[0] + sl[kMsPts]) + sl[2 * kMsPts]) + sl[3 * kMsPts];
      }
      const double pi = s_q[0][p], ql = s_q[1][p], qg = s_q[2][p];
      const double ff = f * f, yi = y[ip];
      const double mi = (1.0 - pi) / mu, ai = (yi - l3[0]) / mu;
      const double dm_l = -ql, da_l = -l3[1];
      const double dm_mu = -((1.0 - 2.0 * pi) + qg) / (mu * mu), da_mu = -(ai - l3[2]) / mu;
      const double aa = ai * ai, ffm = ff * mi;
      t[0] = log(ff / fabs(mi)) + aa / ffm + 1.8378770664093454835606594728112;  // log 2 pi
      t[1] = 2.0 / f - 2.0 * aa / (ffm * f);
      t[2] = -dm_l / mi + 2.0 * ai * da_l / ffm - aa * dm_l / (ffm * mi);
      t[3] = -dm_mu / mi + 2.0 * ai * da_mu / ffm - aa * dm_mu / (ffm * mi);
      t[4] = mi <= 0.0 ? 1.0 : 0.0;  // the counts are exact in a double
      t[5] = outside ? 1.0 : 0.0;
      if (mean_out) mean_out[ip] = yi - ai / mi;
      if (var_out) var_out[ip] = ff / mi;
   }
#pragma unroll
   for (int k = 0; k < kLooSums; k++) {
      double v = t[k];
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) s_red[wave][k] = v;
   }
   __syncthreads();
   if (tid < kLooSums) {
      double v = 0.0;
      for (int w = 0; w < kMsThreads / kWave; w++) v += s_red[w][tid];
      part_out[(size_t)blockIdx.x * kLooSums + tid] = v;
   }
}

// The leave-one-out sums (kLooSums, host) at (f, l, mu) over the bound data; d_mean / d_var (device, n; may be NULL)
// receive the per-point mean and variance.  The object's factor at (l, mu) is fgp_factor's: shared, not rebuilt.
int fgp_loo(FeatureGp* F, double f, double l, double mu, double* d_mean, double* d_var, double* sums)
{
   if (fgp_factor(F, l, mu)) return -1;
   hipStream_t s = current_stream();
   const int Rp = F->Rp, n = F->n;
   const size_t rr = (size_t)Rp * Rp;
   const size_t nblk = ((size_t)n + kMsPts - 1) / kMsPts;
   if (!F->d_looQ) {  // at 128 windows 5 x 170 MB, as long as the object lives
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_looQ, sizeof(double) * 5 * rr));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_loocoef, sizeof(double) * 3 * (size_t)Rp));
   }
   if (nblk + 1 > F->loopart_cap) {
      if (F->d_loopart) (void)hipFree(F->d_loopart);
      F->d_loopart = nullptr;
      F->loopart_cap = 0;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_loopart, sizeof(double) * (nblk + 1) * kLooSums));
      F->loopart_cap = nblk + 1;
   }
   double* V = F->d_vec;
   auto vec = [&](int which) { return (const double*)(V + (size_t)which * Rp); };
   double *Q0 = F->d_looQ, *Ql = Q0 + rr, *Qg = Q0 + 2 * rr, *T1 = Q0 + 3 * rr, *T2 = Q0 + 4 * rr;
   const dim3 g2((Rp + 255) / 256, Rp);
   hipLaunchKernelGGL(k_fgp_loo_mats, g2, dim3(256), 0, s, (const double*)F->d_Binv, vec(kVw), vec(kVdw), Rp, Q0, T1,
                      T2);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (gemm_f64(true, Rp, Rp, Rp, T1, Rp, T2, Rp, Ql, Rp, s)) return -1;  // B^{-1} diag(w') B^{-T}
   hipLaunchKernelGGL(k_fgp_loo_scale, g2, dim3(256), 0, s, (const double*)F->d_Binv, vec(kVw), Rp, T1);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (gemm_f64(false, Rp, Rp, Rp, F->d_G, Rp, T1, Rp, T2, Rp, s)) return -1;  // G P
   if (gemm_f64(true, Rp, Rp, Rp, T1, Rp, T2, Rp, Qg, Rp, s)) return -1;       // P^T G P
   hipLaunchKernelGGL(k_fgp_loo_symmetrise, g2, dim3(256), 0, s, Ql, Rp);
   hipLaunchKernelGGL(k_fgp_loo_symmetrise, g2, dim3(256), 0, s, Qg, Rp);
   hipLaunchKernelGGL(k_fgp_loo_rhs, dim3((Rp + 255) / 256), dim3(256), 0, s, (const double*)F->d_by, vec(kVdw),
                      vec(kVv), vec(kVgv), vec(kVwu), Rp, mu, F->d_loocoef);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   // c_l and c_mu through the factors' substitution, as v is (fgp_factor's note on the residual)
   if (lu_resolve_dev(F->d_B, Rp, F->d_piv, F->d_loocoef + Rp, 2, s)) return -1;
   static const bool attr = []() {
      (void)hipFuncSetAttribute((const void*)k_fgp_loo, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMsLds);
      (void)hipGetLastError();
      return true;
   }();
   (void)attr;
   hipLaunchKernelGGL(k_fgp_loo, dim3((unsigned int)nblk), dim3(kMsThreads), kMsLds, s, (const double*)Q0, Rp,
                      (const double*)F->d_loocoef, (const double*)F->d_centre, (const double*)F->d_scale,
                      (const int*)F->d_feature, F->nw, F->loo_X, F->loo_ld, n, F->loo_y, f, mu, d_mean, d_var,
                      F->d_loopart);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (sum_parts_dev(F->d_loopart, (int)nblk, kLooSums, F->d_loopart + nblk * kLooSums, s)) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(sums, F->d_loopart + nblk * kLooSums, sizeof(double) * kLooSums,
                                    hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   return 0;
}

// what the three leave-one-out entry points refuse alike; 0 when the evaluation may go on
int loo_ready(const FeatureGp* F, const char* who, double f)
{
   if (!F->loo_X || !F->loo_y) {
      fprintf(stderr, "nfft4gp_amd: %s: no data is bound (Nfft4GPAmdFeatureGpLooBind).\n", who);
      return -1;
   }
   if (!std::isfinite(f) || f == 0.0) return -1;
   return 0;
}

int loo_outside(const FeatureGp* F, const char* who, double count)
{
   if (count == 0.0) return 0;
   fprintf(stderr, "nfft4gp_amd: %s: %.0f of %d bound rows lie outside the domain: X is not the data the object was "
                   "created over.\n", who, count, F->n);
   return -1;
}

// the device side of a new object: the handle's windows and the moments of (X, y)
int fgp_fill(FeatureGp* F, const AdditivePlan& P, const char* who, const double* X, int n, int ldim, const double* y)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   const int Rp = F->Rp;
   if (upload(&F->d_centre, P.comp_centre.data(), (size_t)P.nw) ||
       upload(&F->d_scale, P.comp_scale.data(), (size_t)P.nw) ||
       upload(&F->d_feature, P.comp_feature.data(), (size_t)P.nw))
      return -1;
   NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_G, sizeof(double) * (size_t)Rp * Rp));
   NFFT4GP_HIP_CHECK(hipMalloc((void**)&F->d_by, sizeof(double) * ((size_t)Rp + 1)));
   const double *dX, *dy;
   long long ld, ldy;
   if (stage(sc, X, (size_t)n, (size_t)F->d, (size_t)ldim, &dX, &ld) ||
       stage(sc, y, (size_t)n, 1, (size_t)n, &dy, &ldy))
      return -1;
   const WindowMap W = window_map(F);
   long long outside = 0;
   if (window_count_outside(W, dX, ld, n, s, &outside)) return -1;
   if (outside) {
      fprintf(stderr, "%s: %lld of %d rows of X lie outside the handle's domain: X is not the handle's data.\n", who,
              outside, n);
      return -1;
   }
   if (window_moments(W, dX, ld, n, dy, F->d_G, F->d_by, F->d_by + Rp, nullptr, s)) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpy(&F->yy, F->d_by + Rp, sizeof(double), hipMemcpyDeviceToHost));
   return 0;
}

}  // namespace
}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

void* Nfft4GPAmdFeatureGpCreate(void* additive_handle, const double* X, int n, int ldim, int d, const double* y)
{
   const char* who = "nfft4gp_amd: Nfft4GPAmdFeatureGpCreate";
   if (!device_ok()) {
      fprintf(stderr, "%s: no HIP device visible.\n", who);
      return NULL;
   }
   AdditivePlan* Pp = additive_plan_of(additive_handle);
   if (!Pp || !X || !y) {
      fprintf(stderr, "%s needs an additive handle of this library (a distributed operator has none), X and y.\n", who);
      return NULL;
   }
   AdditivePlan& P = *Pp;
   const char* why = nullptr;
   if (!P.points_ready || !P.d_w)
      why = "no Gaussian / Matern-1/2 setup call has been made on the handle";
   else if (P.row_begin != 0 || P.row_end != P.n_global)
      why = "the handle is a row shard";
   else if (P.diag != 1.0 || P.weight != 1.0 / (double)P.nw)
      why = "the handle is a component shard";
   else if (P.md.on || (int)P.comp_feature.size() != P.nw || (int)P.comp_centre.size() != P.nw)
      why = "every window must have exactly one feature";
   else if (n != P.n || n < 1)
      why = "n is not the handle's number of points";
   else if (d != P.d || ldim < n)
      why = "d is not the handle's number of columns, or ldim < n";
   else if (P.nw > kMvMaxNw)
      why = "more than 128 windows (an R x R matrix would exceed 170 MB)";
   if (!why)
      for (int c = 0; c < P.nw; c++)
         if (P.comp_dims[c] != 1 || P.comp_feature[c] < 0 || P.comp_feature[c] >= P.d)
            why = "every window must have exactly one feature";
   if (why) {
      fprintf(stderr, "%s: %s.\n", who, why);
      return NULL;
   }
   FeatureGp* F = new FeatureGp();
   F->n = n;
   F->nw = P.nw;
   F->d = P.d;
   F->kernel = P.kernel;
   F->Rp = mv_order(P.nw);
   F->R = kMvFeat * P.nw;
   F->scale = P.comp_scale;
   if (fgp_fill(F, P, who, X, n, ldim, y)) {
      fgp_free(F);
      return NULL;
   }
   return F;
}

int Nfft4GPAmdFeatureGpSetOptions(void* fgp, nfft4gp_transform_type transform, const int* mask)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || (int)transform < 0 || (int)transform > 3) return -1;
   F->transform = (int)transform;
   F->has_mask = mask != nullptr;
   for (int i = 0; i < 3; i++) F->mask[i] = mask ? mask[i] : 1;
   return 0;
}

int Nfft4GPAmdFeatureGpLoss(void* fgp, double* x, double* lossp, double* dloss)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || !x || !lossp || !dloss) return -1;
   double t[3], dt[3];
   for (int i = 0; i < 3; i++)
      if (Nfft4GPTransform((nfft4gp_transform_type)F->transform, x[i], 0, t + i, dt + i)) return -1;
   const double f = t[0], l = t[1], mu = t[2];
   if (!(mu > 0.0) || !std::isfinite(f) || f == 0.0) return -1;
   if (fgp_factor(F, l, mu)) return -1;
   const double n = (double)F->n, R = (double)F->R, ff = f * f;
   const double bv = F->sc[0], vGv = F->sc[1], uwu = F->sc[2], trBinv = F->sc[3], trBdG = F->sc[4];
   const double q = (F->yy - bv) / mu;                             // y^T M^{-1} y
   const double my2 = (F->yy - 2.0 * bv + vGv) / (mu * mu);        // |M^{-1} y|^2
   const double logdet = n * std::log(ff) + (n - R) * std::log(mu) + F->logabsdet;
   const double loss = 0.5 * (q / (ff * n) + logdet / n + std::log(2.0 * 3.1415926535897932384626));
   const double L1[3] = {2.0 * q / (ff * f) / n, uwu / ff / n, my2 / ff / n};
   const double L2[3] = {2.0 / f, trBdG / n, ((n - R) / mu + trBinv) / n};
   double g[3];
   bool finite = std::isfinite(loss);
   for (int i = 0; i < 3; i++) {
      g[i] = 0.5 * (-L1[i] + L2[i]) * dt[i];
      finite = finite && std::isfinite(g[i]);
      if (F->has_mask && !F->mask[i]) g[i] = 0.0;
   }
   if (!finite) return -1;
   *lossp = loss;
   for (int i = 0; i < 3; i++) dloss[i] = g[i];
   return 0;
}

int Nfft4GPAmdFeatureGpSolve(void* fgp, const double* X, int n, int ldim, int d, const double* y, double f, double l,
                             double mu, double* alpha)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || !X || !y || !alpha || n != F->n || d != F->d || ldim < n || !std::isfinite(f) || f == 0.0) return -1;
   if (fgp_factor(F, l, mu)) return -1;
   const double a = 1.0 / (f * f * mu);
   long long outside = 0;
   if (fgp_apply(F, F->d_vec + (size_t)kVv * F->Rp, X, n, (long long)ldim, y, a, -a, alpha, &outside)) return -1;
   if (outside) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdFeatureGpSolve: %lld of %d rows of X lie outside the domain: X is not the "
                      "data the object was created over.\n", outside, n);
      return -2;
   }
   return 0;
}

int Nfft4GPAmdFeatureGpSolveRhs(void* fgp, const double* X, int n, int ldim, int d, const double* r, double f, double l,
                                double mu, double* alpha)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || !X || !r || !alpha || n != F->n || d != F->d || ldim < n || !std::isfinite(f) || f == 0.0) return -1;
   if (fgp_factor(F, l, mu)) return -1;
   hipStream_t s = current_stream();
   const int Rp = F->Rp;
   Scratch sc(s);
   const double *dX, *dr;
   long long ld, ldr;
   if (stage(sc, X, (size_t)n, (size_t)d, (size_t)ldim, &dX, &ld) || stage(sc, r, (size_t)n, 1, (size_t)n, &dr, &ldr))
      return -1;
   double* tmp;  // Z^T r, r^T r, then v in place of w o Z^T r
   if (sc.alloc(&tmp, 2 * (size_t)Rp + 1)) return -1;
   if (window_moments(window_map(F), dX, ld, n, dr, nullptr, tmp, tmp + Rp, nullptr, s)) return -1;
   double* v = tmp + Rp + 1;
   hipLaunchKernelGGL(k_fgp_hadamard, dim3((Rp + 255) / 256), dim3(256), 0, s, (const double*)F->d_vec,
                      (const double*)tmp, Rp, v);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (lu_resolve_dev(F->d_B, Rp, F->d_piv, v, 1, s)) return -1;
   const double a = 1.0 / (f * f * mu);
   long long outside = 0;
   if (fgp_apply(F, v, dX, n, ld, dr, a, -a, alpha, &outside)) return -1;
   if (outside) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdFeatureGpSolveRhs: %lld of %d rows of X lie outside the domain.\n", outside,
              n);
      return -2;
   }
   return 0;
}

int Nfft4GPAmdFeatureGpVariance(void* fgp, double f, double l, double mu, double* S)
{
   FeatureGp* F = (FeatureGp*)fgp;
   (void)f;  // S does not depend on f: the model applies f^2
   if (!F || !S) return -1;
   if (fgp_factor(F, l, mu)) return -1;
   hipStream_t s = current_stream();
   const int R = F->R;
   Scratch sc(s);
   const bool sdev = is_device_ptr(S);
   double* dS = S;
   if (!sdev && sc.alloc(&dS, (size_t)R * R)) return -1;
   hipLaunchKernelGGL(k_fgp_variance, dim3((R + 255) / 256, R), dim3(256), 0, s, (const double*)F->d_Binv,
                      (const double*)F->d_vec, F->Rp, R, mu, dS);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (!sdev) NFFT4GP_HIP_CHECK(hipMemcpyAsync(S, dS, sizeof(double) * (size_t)R * R, hipMemcpyDeviceToHost, s));
   return sc.finish();
}

int Nfft4GPAmdFeatureGpPredict(void* fgp, double f, double l, double mu, const double* Xnew, int n_new, int ldim, int d,
                               double* mean, long long* n_outside)
{
   FeatureGp* F = (FeatureGp*)fgp;
   (void)f;  // phi^T (w o u) = K(x*, X) A^{-1} y: f^2 cancels
   if (!F || d != F->d || n_new < 0 || ldim < n_new) return -1;
   if (n_outside) *n_outside = 0;
   if (n_new == 0) return 0;
   if (!Xnew || !mean) return -1;
   if (fgp_factor(F, l, mu)) return -1;
   long long outside = 0;
   if (fgp_apply(F, F->d_vec + (size_t)kVwu * F->Rp, Xnew, n_new, (long long)ldim, nullptr, 0.0, 1.0, mean, &outside))
      return -1;
   if (n_outside) *n_outside = outside;
   return 0;
}

int Nfft4GPAmdFeatureGpMoments(void* fgp, double* G, double* b, double* yy)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F) return -1;
   const int Rp = F->Rp, R = F->R;
   if (G) {
      std::vector<double> h((size_t)Rp * Rp);
      NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), F->d_G, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
      for (int i = 0; i < R; i++)
         for (int j = 0; j < R; j++) G[(size_t)i * R + j] = h[(size_t)mv_slot(i) * Rp + mv_slot(j)];
   }
   if (b) {
      std::vector<double> h((size_t)Rp);
      NFFT4GP_HIP_CHECK(hipMemcpy(h.data(), F->d_by, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
      for (int i = 0; i < R; i++) b[i] = h[mv_slot(i)];
   }
   if (yy) *yy = F->yy;
   return 0;
}

int Nfft4GPAmdFeatureGpInfo(void* fgp, int* n, int* nw, int* R, int* kernel)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F) return -1;
   if (n) *n = F->n;
   if (nw) *nw = F->nw;
   if (R) *R = F->R;
   if (kernel) *kernel = F->kernel;
   return 0;
}

int Nfft4GPAmdFeatureGpStatus(void* fgp, int* det_sign, double* logabsdet)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F) return -1;
   if (det_sign) *det_sign = F->det_sign;
   if (logabsdet) *logabsdet = F->logabsdet;
   return 0;
}

int Nfft4GPAmdFeatureGpLooBind(void* fgp, const double* X, int n, int ldim, int d, const double* y)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F) return -1;
   (void)hipStreamSynchronize(current_stream());  // nothing in flight reads the buffers that go
   loo_unbind(F);
   if (!X) return 0;
   if (!y || n != F->n || d != F->d || ldim < n) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAmdFeatureGpLooBind: n and d must be the object's (%d, %d), ldim >= n, and "
                      "y given.\n", F->n, F->d);
      return -1;
   }
   hipStream_t s = current_stream();
   Scratch sc(s);
   const double *dX, *dy;
   long long ld, ldy;
   int rc = stage(sc, X, (size_t)n, (size_t)d, (size_t)ldim, &dX, &ld);
   if (!rc) rc = stage(sc, y, (size_t)n, 1, (size_t)n, &dy, &ldy);
   if (hipStreamSynchronize(s) != hipSuccess) rc = -1;  // the host arrays may go after the call
   if (rc) return rc;                                   // (the copies go with the call; nothing is bound)
   if (dX != X) sc.trade(&F->loo_Xown, (double*)dX);    // the object keeps the copies
   if (dy != y) sc.trade(&F->loo_yown, (double*)dy);
   F->loo_X = dX;
   F->loo_ld = ld;
   F->loo_y = dy;
   return 0;
}

int Nfft4GPAmdFeatureGpLooLoss(void* fgp, double* x, double* lossp, double* dloss)
{
   const char* who = "Nfft4GPAmdFeatureGpLooLoss";
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || !x || !lossp || !dloss) return -1;
   double t[3], dt[3];
   for (int i = 0; i < 3; i++)
      if (Nfft4GPTransform((nfft4gp_transform_type)F->transform, x[i], 0, t + i, dt + i)) return -1;
   const double f = t[0], l = t[1], mu = t[2];
   if (!(mu > 0.0) || loo_ready(F, who, f)) return -1;
   double sums[kLooSums];
   if (fgp_loo(F, f, l, mu, nullptr, nullptr, sums) || loo_outside(F, who, sums[5])) return -1;
   F->loo_nonpositive = (long long)sums[4];
   const double half = 0.5 / (double)F->n;
   const double loss = half * sums[0];
   double g[3];
   bool finite = std::isfinite(loss);
   for (int i = 0; i < 3; i++) {
      g[i] = half * sums[1 + i] * dt[i];
      finite = finite && std::isfinite(g[i]);
      if (F->has_mask && !F->mask[i]) g[i] = 0.0;
   }
   if (!finite) return -1;
   *lossp = loss;
   for (int i = 0; i < 3; i++) dloss[i] = g[i];
   return 0;
}

int Nfft4GPAmdFeatureGpLooPredict(void* fgp, double f, double l, double mu, double* mean, double* var,
                                  long long* n_nonpositive)
{
   const char* who = "Nfft4GPAmdFeatureGpLooPredict";
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || loo_ready(F, who, f)) return -1;
   hipStream_t s = current_stream();
   Scratch sc(s);
   const size_t bytes = sizeof(double) * (size_t)F->n;
   double* host[2] = {mean, var};
   double* dev[2] = {mean, var};
   for (int k = 0; k < 2; k++)
      if (host[k] && !is_device_ptr(host[k]) && sc.alloc(&dev[k], (size_t)F->n)) return -1;
   double sums[kLooSums];
   if (fgp_loo(F, f, l, mu, dev[0], dev[1], sums) || loo_outside(F, who, sums[5])) return -1;
   for (int k = 0; k < 2; k++)
      if (dev[k] != host[k]) NFFT4GP_HIP_CHECK(hipMemcpyAsync(host[k], dev[k], bytes, hipMemcpyDeviceToHost, s));
   F->loo_nonpositive = (long long)sums[4];
   if (n_nonpositive) *n_nonpositive = F->loo_nonpositive;
   return sc.finish();
}

int Nfft4GPAmdFeatureGpLooStatus(void* fgp, long long* n_nonpositive)
{
   FeatureGp* F = (FeatureGp*)fgp;
   if (!F || !n_nonpositive) return -1;
   *n_nonpositive = F->loo_nonpositive;
   return 0;
}

void Nfft4GPAmdFeatureGpFree(void* fgp) { fgp_free((FeatureGp*)fgp); }

}  // extern "C"
