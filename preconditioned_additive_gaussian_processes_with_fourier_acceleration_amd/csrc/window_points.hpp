// window_points.hpp -- what a kernel does with a point in a one-feature window (device code).
// The kernels that walk points over windows (k_model_predict, k_model_effects, k_model_std, k_model_paths,
// k_model_outside, k_model_features, k_model_zty, k_fgp_apply, k_fgp_loo) take from here: the window's angle and its
// 33 trigonometric features, the table's staging and evaluation, the any-window domain test and the workgroup's count
// of outside points.  One text each, so the kernels agree in their bits because they run the same code.
#pragma once
#include "internal.h"

namespace nfft4gp_amd {

// cos and sin of 2 pi xs_q, xs_q the window's quantised coordinate (quantize(): what table_eval decodes its cell and
// offset from); false when the point is outside the window's domain (the angle is then 0)
__device__ inline bool mv_angle(double x, double ctr, double sc, double& c1, double& s1)
{
   const double xs = (x - ctr) * sc;
   const bool in = fabs(xs) <= kMpLimit;
   const double xq = in ? xs : 0.0;
   const uint32_t q = (uint32_t)(unsigned long long)llround(xq * 4294967296.0);
   sincospi((double)(int)q * (1.0 / 2147483648.0), &s1, &c1);  // |xs| <= 1/4: (int)q 2^-32 is xs_q
   return in;
}

// (cos, sin) k theta -> (k + 1) theta: a rotation, whose error grows linearly in k (<= 16 steps)
__device__ inline void mv_rotate(double& ck, double& sk, double c1, double s1)
{
   const double c = ck * c1 - sk * s1;
   sk = sk * c1 + ck * s1;
   ck = c;
}

// The window's 33 features of the coordinate x, in the order cos 0, then (cos k, sin k) for k = 1..16: put(slot, value)
// with slot k for cos k and 16 + k for sin k.  Returns mv_angle's flag.  (k_model_zty and k_fgp_apply interleave their
// points' rotations, four independent chains, and keep loops of their own.)
template <class Put>
__device__ inline bool mv_features(double x, double ctr, double sc, Put&& put)
{
   double c1, s1;
   const bool in = mv_angle(x, ctr, sc, c1, s1);
   double ck = 1.0, sk = 0.0;
#pragma unroll
   for (int k = 0; k <= 16; k++) {
      put(k, ck);
      if (k) put(16 + k, sk);
      mv_rotate(ck, sk, c1, s1);
   }
   return in;
}

// whether row i of X has a coordinate outside some window's domain (NaN and the infinities are outside)
__device__ inline bool row_outside(const double* __restrict__ centre, const double* __restrict__ scale,
                                   const int* __restrict__ feature, int nw, const double* __restrict__ X,
                                   long long ldim, long long i)
{
   bool out = false;
   for (int c = 0; c < nw; c++) {
      const double xs = (X[(size_t)feature[c] * (size_t)ldim + i] - centre[c]) * scale[c];
      out = out || !(fabs(xs) <= kMpLimit);
   }
   return out;
}

// the wave's sum of v in every lane, by a fixed butterfly: the same bits every time (k_model_zty, k_model_effect_moments,
// k_model_intercept_parts)
__device__ inline double zy_wave_sum(double v)
{
#pragma unroll
   for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
   return v;
}

// cnt_out[blockIdx.x] = the workgroup's number of points with bad[p] set, over its kThreads threads' kPts points each
// (a ballot per point, a slot in LDS per wave, thread 0 adds the waves).  Every thread of the workgroup calls it;
// cnt_out may be NULL (uniform): nothing is written then.
template <int kThreads, int kPts>
__device__ inline void block_count_outside(const bool (&bad)[kPts], unsigned int* __restrict__ cnt_out)
{
   __shared__ unsigned int s_cnt[kThreads / kWave];
   const int tid = threadIdx.x;
   if (!cnt_out) return;
   unsigned int cnt = 0;
#pragma unroll
   for (int p = 0; p < kPts; p++) cnt += (unsigned int)__popcll(__ballot(bad[p]));
   if ((tid & (kWave - 1)) == 0) s_cnt[tid / kWave] = cnt;
   __syncthreads();
   if (tid == 0) {
      unsigned int t = 0;
      for (int w = 0; w < kThreads / kWave; w++) t += s_cnt[w];
      cnt_out[blockIdx.x] = t;
   }
}

// ---- the model's table: per window 64 cells of kNC polynomial coefficients ------------------------------------------
constexpr int kMpThreads = 256;          // the workgroup of the kernels that stage the table
constexpr int kMpWin = kNC * kNos + 1;   // staged as [window][degree][cell], windows 513 doubles apart (k_interp_hl)

// ng windows of H ([window][cell][degree], from the group's first window on) into s_H, transposed to
// [window][degree][cell]; the caller's barrier follows
__device__ inline void table_stage(const double* __restrict__ H, int ng, double* s_H)
{
   const double2* src = reinterpret_cast<const double2*>(H);
   const int pairs = ng * kNos * kNC / 2;
   for (int i = threadIdx.x; i < pairs; i += kMpThreads) {
      const double2 v = src[i];
      const int e = 2 * i;  // element of [window][cell][degree]
      double* row = s_H + (e / (kNos * kNC)) * kMpWin + ((e / kNC) & (kNos - 1));
      const int dg = e & (kNC - 1);
      row[dg * kNos] = v.x;
      row[(dg + 1) * kNos] = v.y;
   }
}

// The window's polynomial at the scaled coordinate xs = (x - centre) * scale (subtract, then multiply: the setup's two
// roundings), s_Hw the window's staged rows: the cell / offset decode of the setup, 8 LDS reads and a Horner.  in:
// whether the point is inside the window's domain (false for NaN and the infinities too; the value is then that of
// xs = 0).
__device__ inline double table_eval(const double* s_Hw, double xs, bool& in)
{
   in = fabs(xs) <= kMpLimit;
   const double xq = in ? xs : 0.0;
   const uint32_t q = (uint32_t)(unsigned long long)llround(xq * 4294967296.0);  // quantize()
   const uint32_t cell = q >> 26;
   const double s = (double)(int)(((q & 0x3FFFFFFu) << 6) ^ 0x80000000u);  // slot_word, no index bits
   const double* hrow = s_Hw + cell;
   double hc[kNC];
#pragma unroll
   for (int dg = 0; dg < kNC; dg++) hc[dg] = hrow[dg * kNos];
   double v = hc[kNC - 1];
#pragma unroll
   for (int dg = kNC - 2; dg >= 0; dg--) v = fma(v, s, hc[dg]);
   return v;
}

}  // namespace nfft4gp_amd
