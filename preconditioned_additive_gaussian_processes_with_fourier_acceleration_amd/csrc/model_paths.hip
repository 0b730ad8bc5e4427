// model_paths.hip -- joint posterior sample paths of the fitted model without the training data.
//
// The posterior over functions is finite-rank: f(x) = mean(x) + f phi(x)^T theta, theta ~ N(0, S).  S is not always
// positive semidefinite (W has negative entries), so it is factored by a symmetric eigendecomposition and the negative
// part is dropped: S+ = V max(Lambda, 0) V^T = F F^T, F = V diag(sqrt max(lambda, 0)); defect = sum |lambda < 0| /
// sum |lambda| says how much went.  A set of paths is B = F xi for standard normal xi (R x ns, the caller's), kept in
// the model: the same B evaluated at any point set is the same ns functions.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "model.hpp"
#include "quad_walk.hpp"

namespace nfft4gp_amd {
namespace {

// C[i + j R] = S[slot(i) R_p + slot(j)]: S without its padding (symmetric, so either triangle order)
__global__ void k_model_compact(const double* __restrict__ S, int Rp, int R, double* __restrict__ C)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
   if (i >= R) return;
   C[i + (size_t)j * R] = S[(size_t)mv_slot(i) * Rp + mv_slot(j)];
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
   Scratch sc(s);
   double *V, *Ft, *d_sq;
   if (sc.alloc(&V, (size_t)R * R) || sc.alloc(&Ft, (size_t)R * Rp)) return -1;
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
   if (sc.alloc(&d_sq, sq.size())) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpy(d_sq, sq.data(), sizeof(double) * sq.size(), hipMemcpyHostToDevice));
   hipLaunchKernelGGL(k_model_factor, dim3((R + 255) / 256, Rp), dim3(256), 0, s, (const double*)V, (const double*)d_sq,
                      R, nw, Ft);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   model_drop_sampler(M);  // a refit starts again: the paths of the previous factor go
   sc.trade(&M->d_Ft, Ft);
   M->defect = all > 0.0 ? neg / all : 0.0;
   M->lam_min = w[0];
   M->lam_max = w[R - 1];
   M->sampler_ms = ms;
   return 0;
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
   Scratch sc(s);
   const double* dxi;
   long long ldx;
   if (stage(sc, xi, (size_t)R, (size_t)ns, (size_t)ldxi, &dxi, &ldx)) return -1;
   double* Bt;
   if (sc.alloc(&Bt, (size_t)nsp * Rp)) return -1;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(Bt, 0, sizeof(double) * (size_t)nsp * Rp, s));
   if (gemm_f64(true, ns, Rp, R, dxi, ldx, M->d_Ft, R, Bt, nsp, s)) return -1;
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   sc.trade(&M->d_Bt, Bt);  // the previous paths go with the call
   M->ns = ns;
   M->nsp = nsp;
   return 0;
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
// routes' values within 4.4e-15.  The composed route was removed.
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
   Scratch sc(s);  // the scratch mean is read by the launch in flight: the call always owns it, and always waits
   const double* dX;
   long long ld;
   if (stage(sc, Xnew, (size_t)n_new, (size_t)M->d, (size_t)ldim, &dX, &ld)) return -1;
   double *mean, *oown = nullptr;
   if (sc.alloc(&mean, (size_t)n_new)) return -1;
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
      if (sc.alloc(&oown, (size_t)chunk * ns)) return -1;
   }
   for (long long i0 = 0; i0 < n_new; i0 += chunk) {
      const int cnt = (int)std::min<long long>(chunk, n_new - i0);
      if (launch_paths<kMqBlocks>(M, w0, wn, dX + i0, ld, cnt, mean + i0, odev ? out + i0 : oown,
                                  odev ? ldo : (long long)cnt, s))
         return -1;
      if (!odev) {  // (the next chunk's launch follows the copy on the stream)
         NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(out + i0, sizeof(double) * (size_t)ldo, oown, sizeof(double) * (size_t)cnt,
                                            sizeof(double) * (size_t)cnt, (size_t)ns, hipMemcpyDeviceToHost, s));
         NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
      }
   }
   if (sc.finish()) return -1;
   if (n_outside) *n_outside = outside;
   return 0;
}

}  // namespace
}  // namespace nfft4gp_amd

using namespace nfft4gp_amd;

extern "C" {

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
      const double* row = h.data() + (size_t)mv_slot(i) * R;
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
         B[i + (size_t)sc * R] = h[sc + (size_t)mv_slot(i) * nsp];
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

}  // extern "C"
