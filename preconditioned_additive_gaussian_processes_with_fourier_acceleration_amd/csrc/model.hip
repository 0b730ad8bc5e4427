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
// The table's staging and evaluation and the outside count are window_points.hpp's; the predictive standard deviation
// is model_variance.hip's and the joint posterior's sample paths are model_paths.hip's (model.hpp: what they share).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "model.hpp"
#include "window_points.hpp"

namespace nfft4gp_amd {

void model_drop_sampler(Model* M)
{
   if (M->d_Ft) (void)hipFree(M->d_Ft);
   if (M->d_Bt) (void)hipFree(M->d_Bt);
   M->d_Ft = M->d_Bt = nullptr;
   M->ns = M->nsp = 0;
}

namespace {

constexpr int kMpPts = 4;    // points per thread (strided by the workgroup: coalesced columns)
constexpr int kMpGroup = 8;  // windows staged in LDS per pass (8 x 513 doubles = 32.8 KB)

void model_free(Model* M)
{
   if (!M) return;
   model_drop_sampler(M);
   model_drop_centring(M);
   if (M->d_S) (void)hipFree(M->d_S);
   if (M->d_H) (void)hipFree(M->d_H);
   if (M->d_centre) (void)hipFree(M->d_centre);
   if (M->d_scale) (void)hipFree(M->d_scale);
   if (M->d_feature) (void)hipFree(M->d_feature);
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
      table_stage(H + (size_t)c0 * kNos * kNC, ng, s_H);
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
            bool in;
            acc[p] += table_eval(s_H + cl * kMpWin, (xv[p] - ctr) * sc, in);
            outside[p] = outside[p] || !in;
         }
      }
   }
#pragma unroll
   for (int p = 0; p < kMpPts; p++) {
      const long long i = base + (long long)p * kMpThreads;
      const bool live = i < n_new;
      if (live) mean[i] = outside[p] ? __builtin_nan("") : ff * acc[p];
      outside[p] = live && outside[p];
   }
   block_count_outside<kMpThreads>(outside, cnt_out);
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

// the device side of a model created over a handle: the matvec's own first two steps leave d_H = the table for alpha
// (the interpolation step is the model's)
int model_from_plan(Model* M, AdditivePlan& P, const double* alpha, int n)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   if (model_upload(M, nullptr)) return -1;
   const double* da;
   long long lda;
   if (stage(sc, alpha, (size_t)n, 1, (size_t)n, &da, &lda)) return -1;
   if (launch_spread_grid(P, da, 0, s)) return -1;
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(M->d_H, P.d_H, sizeof(double) * (size_t)P.nw * kNos * kNC, hipMemcpyDeviceToDevice,
                                    s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   return 0;
}

}  // namespace

int model_predict(Model* M, const double* Xnew, int n_new, long long ldim, double* mean, long long* n_outside)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   const double* dX;
   long long ld;
   if (stage(sc, Xnew, (size_t)n_new, (size_t)M->d, (size_t)ldim, &dX, &ld)) return -1;
   const bool mdev = is_device_ptr(mean);
   double* dmean = mean;
   if (!mdev && sc.alloc(&dmean, (size_t)n_new)) return -1;
   const int per = kMpThreads * kMpPts;
   const size_t nblk = ((size_t)n_new + per - 1) / per;
   if (n_outside && M->counts.grow(nblk)) return -1;
   hipLaunchKernelGGL(k_model_predict, dim3((unsigned int)nblk), dim3(kMpThreads), 0, s, (const double*)M->d_H,
                      (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, M->nw, dX, ld,
                      n_new, M->f * M->f, dmean, n_outside ? M->counts.d : (unsigned int*)nullptr);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (!mdev) NFFT4GP_HIP_CHECK(hipMemcpyAsync(mean, dmean, sizeof(double) * (size_t)n_new, hipMemcpyDeviceToHost, s));
   if (n_outside && M->counts.read(nblk, s, n_outside)) return -1;
   return sc.finish();  // with device arrays and no count: nothing to wait for
}

namespace {

// ---- the windows one by one: effect[i][c] = f^2 Horner(H_c), effect_std[i][c] = sqrt| f^2 phi_c^T S_cc phi_c | ------
// f = sum_c g_c is a sum of independent terms a priori; a posteriori g_c(x_c) has mean k_c^T alpha, the value
// k_model_predict adds for window c, and variance f^2 phi_c^T W_c phi_c - k_c^T A^{-1} k_c = f^2 phi_c^T S_cc phi_c,
// S_cc the window's 33 x 33 diagonal block of S (no noise term).  The constant b^_0 / nw sits in every window and only
// the windows' sum of it is identified by the data, so a window's raw std carries the constant's uncertainty.
//
// k_model_effects: k_model_predict's walk (the group's tables staged in LDS, one coalesced coordinate load per
// (point, window), the same table_stage and table_eval) over the windows [w0, w0 + wn), storing each window's ff * v in its
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

//
// kCentred: both about the means over a reference sample.  The window's effect mean is subtracted from
// the rounded product ff * v (two roundings, no contraction across them: the column is the uncentred column minus the
// mean to the bit), and the window's 33 feature means, staged behind the group's S blocks, are subtracted from the
// features once mv_features has delivered the thread's points and before effects_quad, into the registers the
// features occupy anyway: slot 0 is 1 - 1 = 0 exactly, so the constant's variance never enters the form.  The
// <., false> instantiations are instruction for instruction what they were before kCentred existed.
// Measured at n_new = 1e6, 32 windows, alternating with the uncentred passes in one process (tools/
// model_centring_probe.py, profiles/model_centring_probe.json): centred 108.2 us against 99.2 us, with std 1.386 ms
// against 1.295 ms (7.1 %; the run's noise 6.5 us), 167 VGPRs against 164 at the same 3 waves per SIMD.
template <bool kStd, bool kCentred>
__global__ __launch_bounds__(kMpThreads) void k_model_effects(
   const double* __restrict__ H, const double* __restrict__ S, int Rp, const double* __restrict__ centre,
   const double* __restrict__ scale, const int* __restrict__ feature, int w0, int wn, const double* __restrict__ X,
   long long ldim, int n_new, double ff, double* __restrict__ effects, double* __restrict__ effect_std, long long lde,
   long long lds, unsigned int* __restrict__ cnt_out, const double* __restrict__ emean,
   const double* __restrict__ fmean)
{
   constexpr int kPts = kStd ? kMePts : kMpPts;
   constexpr int kGroup = kStd ? kMeGroup : kMpGroup;
   __shared__ double s_H[kGroup * kMpWin];
   __shared__ double s_S[kStd ? kGroup * (kMeBlk + (kCentred ? kMvFeat : 0)) : 1];
   [[maybe_unused]] double* const s_M = s_S + kGroup * kMeBlk;  // with kStd and kCentred: the group's feature means
   const int tid = threadIdx.x;
   const long long base = (long long)blockIdx.x * (kMpThreads * kPts) + tid;
   bool outside[kPts];
#pragma unroll
   for (int p = 0; p < kPts; p++) outside[p] = false;
   for (int c0 = w0; c0 < w0 + wn; c0 += kGroup) {
      const int ng = min(kGroup, w0 + wn - c0);
      if (c0 != w0) __syncthreads();  // every thread has left the previous group's rows
      table_stage(H + (size_t)c0 * kNos * kNC, ng, s_H);
      if constexpr (kStd)
         for (int i = tid; i < ng * kMeBlk; i += kMpThreads) {
            const int cl = i / kMeBlk, e = i - cl * kMeBlk, j = e / kMvFeat, k = e - j * kMvFeat;
            s_S[i] = S[((size_t)(c0 + cl) * kMvPad + j) * Rp + (size_t)(c0 + cl) * kMvPad + k];
         }
      if constexpr (kStd && kCentred)
         for (int i = tid; i < ng * kMvFeat; i += kMpThreads)
            s_M[i] = fmean[(size_t)(c0 + i / kMvFeat) * kMvPad + i % kMvFeat];
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
            const double v = table_eval(s_H + cl * kMpWin, (xv[p] - ctr) * sc, in[p]);
            outside[p] = outside[p] || !in[p];
            if constexpr (kCentred) {
               double e = ff * v;
               asm volatile("" : "+v"(e));  // the product is rounded before the mean is subtracted
               if (effects && i < n_new)
                  effects[(size_t)(c - w0) * (size_t)lde + i] = in[p] ? e - emean[c] : __builtin_nan("");
            } else {
               if (effects && i < n_new)
                  effects[(size_t)(c - w0) * (size_t)lde + i] = in[p] ? ff * v : __builtin_nan("");
            }
         }
         if constexpr (kStd) {
            double phi[kPts][kMvFeat], quad[kPts];
#pragma unroll
            for (int p = 0; p < kPts; p++) {
               (void)mv_features(xv[p], ctr, sc, [&](int j, double v) { phi[p][j] = v; });
               quad[p] = 0.0;
            }
            if constexpr (kCentred) {
               const double* mc = s_M + cl * kMvFeat;
#pragma unroll
               for (int j = 0; j < kMvFeat; j++) {
                  const double mj = mc[j];  // a broadcast read, shared by the thread's points
#pragma unroll
                  for (int p = 0; p < kPts; p++) {
                     // phi - m in the feature's own register pair.  Written as phi[p][j] -= mj the allocator gives
                     // every difference a fresh pair while the features are still live: 195 VGPRs and 2 waves per
                     // SIMD; tied to its source it is 167 and 3, the uncentred kernel's shape.
                     asm volatile("v_add_f64 %0, %0, -%1" : "+v"(phi[p][j]) : "v"(mj));
                  }
                  if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);  // at most 8 means in flight (effects_quad's rule)
               }
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
               if (i < n_new)
                  effect_std[(size_t)(c - w0) * (size_t)lds + i] = in[p] ? sqrt(fabs(ff * quad[p])) : __builtin_nan("");
            }
         }
      }
   }
#pragma unroll
   for (int p = 0; p < kPts; p++) outside[p] = outside[p] && base + (long long)p * kMpThreads < n_new;
   block_count_outside<kMpThreads>(outside, cnt_out);
}

}  // namespace

int model_predict_effects(Model* M, const double* Xnew, int n_new, long long ldim, int w0, int wn, double* effects,
                          double* effect_std, long long ldo, long long* n_outside, bool centred)
{
   hipStream_t s = current_stream();
   Scratch sc(s);
   const size_t col = sizeof(double) * (size_t)n_new;
   const double* dX = Xnew;
   long long ld = ldim;
   if (!is_device_ptr(Xnew)) {  // only the columns the windows in range read (stage() would copy all d)
      double* xown;
      if (sc.alloc(&xown, (size_t)n_new * M->d)) return -1;
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
      if (sc.alloc(&de, (size_t)n_new * wn)) return -1;
      lde = n_new;
   }
   if (shost) {
      if (sc.alloc(&ds, (size_t)n_new * wn)) return -1;
      lds = n_new;
   }
   const int per = kMpThreads * (effect_std ? kMePts : kMpPts);
   const size_t nblk = ((size_t)n_new + per - 1) / per;
   if (n_outside && M->counts.grow(nblk)) return -1;
   unsigned int* cnt = n_outside ? M->counts.d : (unsigned int*)nullptr;
   const dim3 grid((unsigned int)nblk), block(kMpThreads);
   auto* kern = effect_std ? (centred ? k_model_effects<true, true> : k_model_effects<true, false>)
                           : (centred ? k_model_effects<false, true> : k_model_effects<false, false>);
   hipLaunchKernelGGL(kern, grid, block, 0, s, (const double*)M->d_H, (const double*)M->d_S, mv_order(M->nw),
                      (const double*)M->d_centre, (const double*)M->d_scale, (const int*)M->d_feature, w0, wn, dX, ld,
                      n_new, M->f * M->f, de, ds, lde, lds, cnt, (const double*)M->d_emean, (const double*)M->d_fmean);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (ehost)
      NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(effects, sizeof(double) * (size_t)ldo, de, col, col, (size_t)wn,
                                         hipMemcpyDeviceToHost, s));
   if (shost)
      NFFT4GP_HIP_CHECK(hipMemcpy2DAsync(effect_std, sizeof(double) * (size_t)ldo, ds, col, col, (size_t)wn,
                                         hipMemcpyDeviceToHost, s));
   if (n_outside && M->counts.read(nblk, s, n_outside)) return -1;
   return sc.finish();
}

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
   const int rc = model_from_plan(M, P, alpha, n);
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

void Nfft4GPAmdModelFree(void* model) { model_free((Model*)model); }

}  // extern "C"
