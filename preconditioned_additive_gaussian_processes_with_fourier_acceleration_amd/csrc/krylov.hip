// krylov.hip -- the device side of the Krylov solvers (fgmres.hip, lanczos.hip, gp_loss.hip), with every n-vector
// (Krylov bases, iterates, probes) in HBM: every Gram-Schmidt and vector kernel, their scratch (KScratch) and the
// launch code (Ctx, BatchCtx: krylov.hpp) -- the only place these kernels are launched from.
//
//   k_gs_step, k_mgs_chain, k_mgs_wide   Nfft4GPModifiedGS   SRC/linearalg/matops.c:274-346 (FGMRES's sweep)
//   k_block_dots, k_block_update,        Nfft4GPModifiedGS2  matops.c:348-440 (the Lanczos re-orthogonalisation,
//   k_lanczos_local                                          as classical passes with the DGKS test)
//
// Each Gram-Schmidt step is one fused launch (apply the previous projection, then the next inner product, reduced
// on the device in a fixed order: reduce.hpp's summed inner products); the one-launch sweeps run a whole step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "krylov.hpp"
#include "reduce.hpp"

using namespace nfft4gp_amd;

namespace {

constexpr int kKThreads = 256;
constexpr int kKEPT = 4;
constexpr int kKMaxBlocks = 2048;  // <= kRedMaxBlocks

int kgrid(size_t n)
{
   size_t g = (n + (size_t)kKThreads * kKEPT - 1) / ((size_t)kKThreads * kKEPT);
   g = std::min<size_t>(g, kKMaxBlocks);
   return (int)(g == 0 ? 1 : g);
}

// the grid of the 1024-thread x 4-element kernels (k_gs_step, k_gs_batch and the one-launch sweeps)
unsigned gs_grid(size_t n)
{
   return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 4095) / 4096, kKMaxBlocks));
}

// workgroups of 1024 threads of `kernel` that are resident on the device at once (occupancy x CUs); 0: unknown
template <class K>
int resident_workgroups(K kernel)
{
   int dev = 0, occ = 0;
   hipDeviceProp_t prop;
   if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
       hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 1024, 0) == hipSuccess)
      return occ * prop.multiProcessorCount;
   return 0;
}

// w -= (*hprev) * u (when u != nullptr); then *out = (w, v) (v != nullptr) or ||w||^2 (v == nullptr).
// T threads per block: 1024 gives a quarter of the partials for the last block to add (the MGS loop of
// FGMRES runs one of these per projection, so its serial tail is most of a step at n = 1e6).
template <int T, int EPT>
__device__ __forceinline__ void gs_body(double* __restrict__ w, const double* __restrict__ u, double h,
                                        const double* __restrict__ v, size_t n, double* __restrict__ part,
                                        unsigned int* __restrict__ ticket, double* __restrict__ out)
{
   double acc = 0.0;
   const size_t stride = (size_t)gridDim.x * T * EPT;
   for (size_t i0 = (size_t)blockIdx.x * T * EPT + threadIdx.x; i0 < n; i0 += stride) {
      double wv[EPT], uv[EPT], vv[EPT];
#pragma unroll
      for (int e = 0; e < EPT; e++) {
         const size_t i = i0 + (size_t)e * T;
         wv[e] = i < n ? w[i] : 0.0;
         uv[e] = (u && i < n) ? u[i] : 0.0;
         vv[e] = (v && i < n) ? v[i] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < EPT; e++) {
         const size_t i = i0 + (size_t)e * T;
         if (u) {
            wv[e] = fma(-h, uv[e], wv[e]);
            if (i < n) w[i] = wv[e];
         }
         acc = v ? fma(wv[e], vv[e], acc) : fma(wv[e], wv[e], acc);
      }
   }
   acc = block_sum0<T>(acc);
   double tot;
   if (grid_total<T>(acc, part, ticket, &tot) && threadIdx.x == 0) *out = tot;
}

template <int T, int EPT = kKEPT>
__global__ __launch_bounds__(T) void k_gs_step(double* __restrict__ w, const double* __restrict__ u,
                                               const double* __restrict__ hprev, const double* __restrict__ v,
                                               size_t n, double* __restrict__ part, unsigned int* __restrict__ ticket,
                                               double* __restrict__ out)
{
   gs_body<T, EPT>(w, u, u ? *hprev : 0.0, v, n, part, ticket, out);
}

// k_gs_step for several systems of one batch at once (the predict's std solves, fgmres_batch_dev): blockIdx.y
// runs system s = act[y], whose operands sit ld* doubles apart (w + s ldw, ...), its scalars at hprev[s] and
// out[s]; one partials / ticket pair per y.  Per system the arithmetic is k_gs_step's (same grid): bitwise.
template <int T, int EPT>
__global__ __launch_bounds__(T) void k_gs_batch(double* __restrict__ w, size_t ldw, const double* __restrict__ u,
                                                size_t ldu, const double* __restrict__ hprev,
                                                const double* __restrict__ v, size_t ldv, size_t n,
                                                const int* __restrict__ act, double* __restrict__ part,
                                                unsigned int* __restrict__ ticket, double* __restrict__ out)
{
   const int s = act[blockIdx.y];
   gs_body<T, EPT>(w + (size_t)s * ldw, u ? u + (size_t)s * ldu : nullptr, u ? hprev[s] : 0.0,
                   v ? v + (size_t)s * ldv : nullptr, n, part + (size_t)blockIdx.y * kKMaxBlocks,
                   ticket + (size_t)blockIdx.y * kTicketWords, out + s);
}

// The whole MGS sweep of one FGMRES step in ONE launch (Nfft4GPModifiedGS, matops.c:274-346, as the chain of
// k_gs_step launches Ctx::gs makes): w stays in registers across the i projections and the norm, each step
// reads only v_j (v_{j-1}, the previous step's u, is still in registers; v_{j+1}'s loads go out before the
// step's wait), and the grid-wide sum of step j (reduce.hpp's last arriver) reaches every workgroup through
// hd[j] itself: the host presets hd[0..i] to an all-ones NaN pattern (kChainUnset) that no sum of finite data
// produces, the last arriver stores the sum there (agent scope, after its ticket resets have landed) and the
// others poll it until it changes -- no fences, as reduce.hpp.  Needs a grid that is resident at once and covers
// n in one pass (the host checks the occupancy).  Per element and per reduction the arithmetic is k_gs_step's on
// the same grid, so hd[0..i] and w are bitwise the chain's.  A wait that gives up sets *err (host: an error).
// BATCH (fgmres_batch_dev, the predict's std solves): blockIdx.y runs system s = act[y] of a batch of m, whose
// column j is cols[j] + s n (w: column i), its scalars at hd[j m + s], one partials / ticket pair per y
constexpr unsigned long long kChainUnset = ~0ull;  // hd[j] before step j's sum is published

// The one-launch kernels' hand-off of a grid-wide sum through its preset slot (one thread of the workgroup).
// The last arriver publishes: its ticket resets land first (vmcnt(0)), then one relaxed agent-scope store.
__device__ __forceinline__ void chain_publish(double* slot, double tot)
{
   asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the ticket resets land before the publish
   __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(tot),
                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Everyone else polls the slot until it changes, a bounded number of times: true with the sum in *val, or false
// after setting *s_fail (the workgroup leaves after its barrier) and *err (the host fails the solve)
__device__ __forceinline__ bool chain_wait(double* slot, double* val, int* s_fail, int* err)
{
   unsigned long long* sl = reinterpret_cast<unsigned long long*>(slot);
   unsigned long long b = kChainUnset;
   for (long spin = 0; spin < (1l << 22); spin++) {
      b = __hip_atomic_load(sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (b != kChainUnset) break;
      __builtin_amdgcn_s_sleep(1);
   }
   if (b == kChainUnset) {
      *s_fail = 1;
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
   }
   *val = __longlong_as_double((long long)b);
   return true;
}

template <int T, int EPT, bool BATCH = false>
__global__ __launch_bounds__(T) void k_mgs_chain(double* __restrict__ w, const double* __restrict__ V, size_t n,
                                                 int i, double* __restrict__ hd, double* __restrict__ part,
                                                 unsigned int* __restrict__ ticket,
                                                 int* __restrict__ err, const double* const* __restrict__ cols = nullptr,
                                                 const int* __restrict__ act = nullptr, int m = 1)
{
   __shared__ double s_h;
   __shared__ int s_fail;
   int hs = 1;  // hd stride between steps
   if (BATCH) {
      const int sy = act[blockIdx.y];
      w = const_cast<double*>(cols[i]) + (size_t)sy * n;
      hd += sy;
      hs = m;
      part += (size_t)blockIdx.y * kKMaxBlocks;
      ticket += (size_t)blockIdx.y * kTicketWords;
   }
   auto col = [&](int j) -> const double* {
      return BATCH ? cols[j] + (size_t)act[blockIdx.y] * n : V + (size_t)j * n;
   };
   const size_t i0 = (size_t)blockIdx.x * T * EPT + threadIdx.x;
   double wv[EPT], pv[EPT], vn[EPT];
   const double* v0 = i > 0 ? col(0) : nullptr;
#pragma unroll
   for (int e = 0; e < EPT; e++) {
      const size_t k = i0 + (size_t)e * T;
      wv[e] = k < n ? w[k] : 0.0;
      pv[e] = 0.0;
      vn[e] = (v0 && k < n) ? v0[k] : 0.0;  // v_0
   }
   if (threadIdx.x == 0) s_fail = 0;
   for (int j = 0; j <= i; j++) {
      if (j > 0) {
         const double h = s_h;
#pragma unroll
         for (int e = 0; e < EPT; e++) wv[e] = fma(-h, pv[e], wv[e]);
      }
      double acc = 0.0;
      if (j < i) {
         double vv[EPT];
#pragma unroll
         for (int e = 0; e < EPT; e++) vv[e] = vn[e];
         // v_{j+1}'s loads go out now: they do not depend on this step's sum, so they overlap its grid-wide wait
         if (j + 1 < i) {
            const double* v1 = col(j + 1);
#pragma unroll
            for (int e = 0; e < EPT; e++) {
               const size_t k = i0 + (size_t)e * T;
               vn[e] = k < n ? v1[k] : 0.0;
            }
         }
#pragma unroll
         for (int e = 0; e < EPT; e++) {
            acc = fma(wv[e], vv[e], acc);
            pv[e] = vv[e];
         }
      } else {
#pragma unroll
         for (int e = 0; e < EPT; e++) acc = fma(wv[e], wv[e], acc);
      }
      acc = block_sum0<T>(acc);
      double tot;
      double* slot = hd + (size_t)j * hs;
      if (grid_total<T>(acc, part, ticket, &tot)) {
         if (threadIdx.x == 0) {
            chain_publish(slot, tot);
            s_h = tot;
         }
      } else if (threadIdx.x == 0) {
         chain_wait(slot, &s_h, &s_fail, err);
      }
      __syncthreads();
      if (s_fail) return;  // the others time out at the next step in turn
   }
#pragma unroll
   for (int e = 0; e < EPT; e++) {
      const size_t k = i0 + (size_t)e * T;
      if (k < n) w[k] = wv[e];
   }
}

// The MGS sweep in ONE launch for vectors too long for k_mgs_chain's one-pass grid (config E, n = 1e7): w stays
// in registers across the whole sweep -- S strided passes of 4 elements per thread, exactly the elements and the
// order k_gs_step<1024, 4> visits on the same grid -- while v_{j-1} is re-read for each update instead of being
// held (w, v_{j-1} and v_j would not fit the register file at this n).  Step j: w -= h_{j-1} v_{j-1}, then
// (w, v_j) (the last step ||w||^2), summed by reduce.hpp's last arriver and published into the preset hd[j] as
// k_mgs_chain does (bounded waits, *err).  Per element and per reduction the arithmetic of the per-projection
// chain on this grid (Ctx::mgs_grid): bitwise equal to it.  Moves 2 vectors per projection against the chain's
// 4 (w read and written, v_{j-1}, v_j).
template <int T, int S>
__global__ __launch_bounds__(T) void k_mgs_wide(double* __restrict__ w, const double* __restrict__ V, size_t n, int i,
                                                double* __restrict__ hd, double* __restrict__ part,
                                                unsigned int* __restrict__ ticket, int* __restrict__ err)
{
   constexpr int E = 4;
   __shared__ double s_h;
   __shared__ int s_fail;
   // element (p, e) of this thread is c(p, e) + threadIdx.x with c wave-uniform: the loads take a scalar base and
   // one 32-bit lane offset, so no per-element 64-bit address stays live across the sweep
   const size_t stride = (size_t)gridDim.x * T * E;
   const size_t c0 = (size_t)blockIdx.x * T * E;
   const unsigned tid = threadIdx.x;
   auto cbase = [&](int p, int e) -> size_t { return c0 + (size_t)p * stride + (size_t)e * T; };
   double wv[S][E];
#pragma unroll
   for (int p = 0; p < S; p++)
#pragma unroll
      for (int e = 0; e < E; e++) {
         const size_t c = cbase(p, e);
         wv[p][e] = c + tid < n ? (w + c)[tid] : 0.0;
      }
   if (threadIdx.x == 0) s_fail = 0;
   for (int j = 0; j <= i; j++) {
      const double* u = j > 0 ? V + (size_t)(j - 1) * n : nullptr;
      const double* v = j < i ? V + (size_t)j * n : nullptr;
      const double h = j > 0 ? s_h : 0.0;
      double acc = 0.0;
#pragma unroll
      for (int p = 0; p < S; p++) {
         if (cbase(p, 0) + tid < n) {  // gs_body's grid-stride loop has ended for this thread past here
            double uv[E], vv[E];
#pragma unroll
            for (int e = 0; e < E; e++) {
               const size_t c = cbase(p, e);
               const bool in = c + tid < n;
               uv[e] = (u && in) ? (u + c)[tid] : 0.0;
               vv[e] = (v && in) ? (v + c)[tid] : 0.0;
            }
#pragma unroll
            for (int e = 0; e < E; e++) {
               if (u) wv[p][e] = fma(-h, uv[e], wv[p][e]);
               acc = v ? fma(wv[p][e], vv[e], acc) : fma(wv[p][e], wv[p][e], acc);
            }
         }
         // one pass's 8 loads in flight per thread: hoisting every pass's loads above the arithmetic would need
         // 16 S VGPRs beside w's 8 S
         asm volatile("" ::: "memory");
      }
      acc = block_sum0<T>(acc);
      double tot;
      double* slot = hd + j;
      if (grid_total<T>(acc, part, ticket, &tot)) {
         if (threadIdx.x == 0) {
            chain_publish(slot, tot);
            s_h = tot;
         }
      } else if (threadIdx.x == 0) {
         chain_wait(slot, &s_h, &s_fail, err);
      }
      __syncthreads();
      if (s_fail) return;
   }
#pragma unroll
   for (int p = 0; p < S; p++)
#pragma unroll
      for (int e = 0; e < E; e++) {
         const size_t c = cbase(p, e);
         if (c + tid < n) (w + c)[tid] = wv[p][e];
      }
}

// k_mgs_wide's instantiations: passes S per thread
constexpr int kWideS[] = {2, 4, 6, 8, 10, 12};
typedef void (*MgsWideFn)(double*, const double*, size_t, int, double*, double*, unsigned int*, int*);
static MgsWideFn mgs_wide_fn(int S)
{
   switch (S) {
   case 2: return k_mgs_wide<1024, 2>;
   case 4: return k_mgs_wide<1024, 4>;
   case 6: return k_mgs_wide<1024, 6>;
   case 8: return k_mgs_wide<1024, 8>;
   case 10: return k_mgs_wide<1024, 10>;
   case 12: return k_mgs_wide<1024, 12>;
   default: return nullptr;
   }
}

// mgs2's local pass in ONE launch (what Ctx::block_gs(w, V + j0 n, Z + j0 n, ml, h, 1) does in three: h[0..ml) =
// [v_j0, v_j0+1]^T w, h[ml + 1] = ||w||^2 before, w -= Z_loc h, h[ml] = ||w||^2 after).  The ml + 1 grid-wide sums
// of the first half are reduce.hpp's last-arriver sums (one partials / ticket pair each), published into hd
// slots the host preset to kChainUnset; every workgroup waits for the projections (bounded), updates its w
// and forms the norm after, whose last arriver writes hd[ml].  alias: Z_loc == V_loc (no preconditioner), so
// the update reuses the loaded columns.  The same sums as block_gs's up to their order (rounding level).
template <int T, int EPT>
__global__ __launch_bounds__(T) void k_lanczos_local(double* __restrict__ w, const double* __restrict__ V0,
                                                     const double* __restrict__ Z0, int alias, size_t n, int ml,
                                                     double* __restrict__ hd, double* __restrict__ part,
                                                     unsigned int* __restrict__ ticket, int* __restrict__ err)
{
   __shared__ double s_sc[3][T / 64];
   __shared__ int s_last[3];
   __shared__ double s_h[2];
   __shared__ int s_fail;
   const size_t i0 = (size_t)blockIdx.x * T * EPT + threadIdx.x;
   double wv[EPT], v0[EPT], v1[EPT];
#pragma unroll
   for (int e = 0; e < EPT; e++) {
      const size_t k = i0 + (size_t)e * T;
      const bool in = k < n;
      wv[e] = in ? w[k] : 0.0;
      v0[e] = in ? V0[k] : 0.0;
      v1[e] = (in && ml == 2) ? V0[n + k] : 0.0;
   }
   double a0 = 0.0, a1 = 0.0, an = 0.0;
#pragma unroll
   for (int e = 0; e < EPT; e++) {
      a0 = fma(wv[e], v0[e], a0);
      a1 = fma(wv[e], v1[e], a1);
      an = fma(wv[e], wv[e], an);
   }
   if (threadIdx.x == 0) s_fail = 0;
   const double sums[3] = {a0, a1, an};
   // hd slots: [0] (w, v_j0), [1] (w, v_j0+1) when ml == 2, [ml + 1] ||w||^2 before
   const int slot_of[3] = {0, 1, ml + 1};
#pragma unroll
   for (int q = 0; q < 3; q++) {
      if (q == 1 && ml != 2) continue;
      double b = block_sum0_s<T>(sums[q], s_sc[q]);
      double tot;
      if (grid_total_s<T>(b, part + (size_t)q * kKMaxBlocks, ticket + (size_t)q * kTicketWords, &tot, &s_last[q],
                          s_sc[q]) &&
          threadIdx.x == 0)
         chain_publish(hd + slot_of[q], tot);
      __syncthreads();
   }
   if (threadIdx.x == 0) {
      for (int j = 0; j < ml; j++)
         if (!chain_wait(hd + j, &s_h[j], &s_fail, err)) break;
   }
   __syncthreads();
   if (s_fail) return;
   const double h0 = s_h[0], h1 = ml == 2 ? s_h[1] : 0.0;
   double acc = 0.0;
#pragma unroll
   for (int e = 0; e < EPT; e++) {
      const size_t k = i0 + (size_t)e * T;
      const bool in = k < n;
      const double z0 = alias ? v0[e] : (in ? Z0[k] : 0.0);
      const double z1 = ml == 2 ? (alias ? v1[e] : (in ? Z0[n + k] : 0.0)) : 0.0;
      wv[e] = fma(-h0, z0, wv[e]);
      if (ml == 2) wv[e] = fma(-h1, z1, wv[e]);
      if (in) w[k] = wv[e];
      acc = fma(wv[e], wv[e], acc);
   }
   // the norm after: tickets of pair 0 again (every workgroup is past that pair's publish, so its reset landed)
   const double b = block_sum0_s<T>(acc, s_sc[0]);
   double tot;
   if (grid_total_s<T>(b, part + 3 * (size_t)kKMaxBlocks, ticket, &tot, &s_last[0], s_sc[0]) && threadIdx.x == 0)
      hd[ml] = tot;
}

// a[s] *= fac[s] for the systems act[y] (k_scale2's arithmetic)
__global__ void k_scale_batch(double* __restrict__ a, size_t lda, size_t n, const int* __restrict__ act,
                              const double* __restrict__ fac)
{
   const int s = act[blockIdx.y];
   const double f = fac[s];
   double* p = a + (size_t)s * lda;
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] *= f;
}

// x += sum_j c[j] cols[j] (columns in order: k_combine's arithmetic over columns that need not be contiguous)
__global__ void k_combine_cols(double* __restrict__ x, const double* const* __restrict__ cols, size_t n,
                               const double* __restrict__ c, int m)
{
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
      double v = x[i];
      for (int j = 0; j < m; j++) v = fma(c[j], cols[j][i], v);
      x[i] = v;
   }
}


// out[0] = (a, b), out[1] = (b, b): the Lanczos (v, z) and ||z||^2 in one pass
__global__ __launch_bounds__(kKThreads) void k_dot2(const double* __restrict__ a, const double* __restrict__ b,
                                                    size_t n, double* __restrict__ part,
                                                    unsigned int* __restrict__ ticket, double* __restrict__ part2,
                                                    unsigned int* __restrict__ ticket2, double* __restrict__ out)
{
   double ab = 0.0, bb = 0.0;
   const size_t stride = (size_t)gridDim.x * kKThreads * kKEPT;
   for (size_t i0 = (size_t)blockIdx.x * kKThreads * kKEPT + threadIdx.x; i0 < n; i0 += stride) {
      double av[kKEPT], bv[kKEPT];
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         const size_t i = i0 + (size_t)e * kKThreads;
         av[e] = i < n ? a[i] : 0.0;
         bv[e] = i < n ? b[i] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         ab = fma(av[e], bv[e], ab);
         bb = fma(bv[e], bv[e], bb);
      }
   }
   ab = block_sum0<kKThreads>(ab);
   double tot;
   if (grid_total<kKThreads>(ab, part, ticket, &tot) && threadIdx.x == 0) out[0] = tot;
   __syncthreads();
   bb = block_sum0<kKThreads>(bb);
   if (grid_total<kKThreads>(bb, part2, ticket2, &tot) && threadIdx.x == 0) out[1] = tot;
}

__global__ void k_scale2(double* __restrict__ a, double* __restrict__ b, size_t n, double s)
{
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
      a[i] *= s;
      if (b) b[i] *= s;
   }
}

// x += sum_j c[j] B[:, j] (columns in order, ld = n)
__global__ void k_combine(double* __restrict__ x, const double* __restrict__ B, size_t ld, size_t n,
                          const double* __restrict__ c, int m)
{
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
      double v = x[i];
      for (int j = 0; j < m; j++) v = fma(c[j], B[(size_t)j * ld + i], v);
      x[i] = v;
   }
}

// y = a - b
__global__ void k_sub(double* __restrict__ y, const double* __restrict__ a, const double* __restrict__ b, size_t n)
{
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
      y[i] = a[i] - b[i];
}

// ---- block (classical) Gram-Schmidt passes for the Lanczos re-orthogonalisation -------------------
// One pass = two launches over the whole basis: h = V^T w (kBD basis vectors per workgroup, every
// block's partials reduced in a fixed order), then w -= Z h with ||w||^2 fused.  This reads the basis
// twice per pass instead of streaming w, z_i and v_i once per basis vector (MGS: 4 vectors moved per
// projection): 2x fewer bytes and 2 launches instead of k + 2.
constexpr int kBD = 8;
constexpr int kBDThreads = 256;
constexpr int kBDMaxBlocks = 512;

int bd_grid(size_t n)
{
   size_t g = (n + (size_t)kBDThreads * 16 - 1) / ((size_t)kBDThreads * 16);
   return (int)std::max<size_t>(1, std::min<size_t>(g, kBDMaxBlocks));
}

// part[blockIdx.x * ldp + i] = sum over this block's rows r of w[r] V[i n + r], i in [g0, g0 + kBD) & < m;
// with_norm: column m is w itself (part[.. + m] sums ||w||^2)
// c_after / c_before (optional): a second pass that runs only when the DGKS test of k_block_update holds
// FOLD: k_block_reduce folded in -- the partials are stored at agent scope, the last arriving workgroup of each
// column group (reduce.hpp's per-XCD tickets, one ticket array per group) sums them in k_block_reduce's order
// and writes h[0..m) (h[m + 1] for the norm column): one launch instead of two, the same bits
// VEC = 2: each thread reads two consecutive rows per column as one 16-byte load (the host picks it when n is even
// and w, V are 16-byte aligned, so every column is)
template <bool FOLD = false, int VEC = 1>
__global__ __launch_bounds__(kBDThreads) void k_block_dots(const double* __restrict__ w, const double* __restrict__ V,
                                                           size_t n, int m, int with_norm, double* __restrict__ part,
                                                           int ldp, const double* __restrict__ c_after = nullptr,
                                                           const double* __restrict__ c_before = nullptr,
                                                           double* __restrict__ h = nullptr,
                                                           unsigned int* __restrict__ tickets = nullptr)
{
   if (c_after && !(sqrt(*c_after) < 0.7071 * sqrt(*c_before))) return;
   __shared__ double s[kBDThreads / 64][kBD];
   const int g0 = blockIdx.y * kBD;
   const int cnt = min(kBD, m + with_norm - g0);
   const int nv = m - g0;  // columns of this group that come from V; the next one (if counted) is w
   double acc[kBD];
#pragma unroll
   for (int j = 0; j < kBD; j++) acc[j] = 0.0;
   const size_t stride = (size_t)gridDim.x * kBDThreads;
   if constexpr (VEC == 1) {
      for (size_t r = (size_t)blockIdx.x * kBDThreads + threadIdx.x; r < n; r += stride) {
         const double wr = w[r];
         double v[kBD];
#pragma unroll
         for (int j = 0; j < kBD; j++) v[j] = j < nv && j < cnt ? V[(size_t)(g0 + j) * n + r] : (j < cnt ? wr : 0.0);
#pragma unroll
         for (int j = 0; j < kBD; j++) acc[j] = fma(v[j], wr, acc[j]);
      }
   } else {
      const size_t n2 = n / 2;
      const double2* __restrict__ w2 = reinterpret_cast<const double2*>(w);
      for (size_t r = (size_t)blockIdx.x * kBDThreads + threadIdx.x; r < n2; r += stride) {
         const double2 wr = w2[r];
         double2 v[kBD];
#pragma unroll
         for (int j = 0; j < kBD; j++)
            v[j] = j < nv && j < cnt ? reinterpret_cast<const double2*>(V + (size_t)(g0 + j) * n)[r]
                                     : (j < cnt ? wr : make_double2(0.0, 0.0));
#pragma unroll
         for (int j = 0; j < kBD; j++) acc[j] = fma(v[j].y, wr.y, fma(v[j].x, wr.x, acc[j]));
      }
   }
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
   for (int j = 0; j < kBD; j++) {
      double a = acc[j];
      for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
      if (lane == 0) s[wave][j] = a;
   }
   __syncthreads();
   if (threadIdx.x < cnt) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < kBDThreads / 64; q++) t += s[q][threadIdx.x];
      if (FOLD)
         __hip_atomic_store(part + (size_t)blockIdx.x * ldp + g0 + threadIdx.x, t, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
      else
         part[(size_t)blockIdx.x * ldp + g0 + threadIdx.x] = t;
   }
   if constexpr (FOLD) {
      __shared__ int s_last;
      __shared__ double s_sum[16][kBD];
      unsigned int* ticket = tickets + (size_t)blockIdx.y * kTicketWords;
      if (threadIdx.x == 0) {  // the partial stores are wave 0's (cnt <= kBD lanes)
         asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
         const unsigned G = gridDim.x;
         const unsigned xcd = blockIdx.x % kRedXcds;
         const unsigned members = (G - xcd + kRedXcds - 1) / kRedXcds;
         const unsigned groups = G < kRedXcds ? G : kRedXcds;
         int last = 0;
         const unsigned old = __hip_atomic_fetch_add(ticket + (1 + xcd) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
         if (old == members - 1) {
            const unsigned top = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (top == groups - 1);
         }
         s_last = last;
      }
      __syncthreads();
      if (!s_last) return;
      // k_block_reduce's sum: 16 strands per column, four accumulators cycled, then the strands in order
      const int col = threadIdx.x % kBD, g = threadIdx.x / kBD;
      if (g < 16) {
         double z[4] = {0.0, 0.0, 0.0, 0.0};
         int u = 0;
         const int nblk = (int)gridDim.x;
         const int ii = col < cnt ? g0 + col : g0 + cnt - 1;
         for (int b = g; b < nblk; b += 16, u = (u + 1) & 3)
            z[u] += __hip_atomic_load(part + (size_t)b * ldp + ii, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         s_sum[g][col] = (z[0] + z[1]) + (z[2] + z[3]);
      }
      __syncthreads();
      if (threadIdx.x < cnt) {
         double t = 0.0;
#pragma unroll
         for (int q = 0; q < 16; q++) t += s_sum[q][threadIdx.x];
         const int i = g0 + threadIdx.x;
         h[i < m ? i : m + 1] = t;
      }
      if (threadIdx.x <= (unsigned)kRedXcds)
         __hip_atomic_store(ticket + threadIdx.x * kTicketStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
   }
}

// h[i] = sum_b part[b ldp + i] (fixed order: 16 strands over blocks b = g mod 16, then the strands) for
// i < m; column i = m (the norm column of k_block_dots, when mc = m + 1) lands in h[m + 1]
__global__ __launch_bounds__(1024) void k_block_reduce(const double* __restrict__ part, int nblk, int ldp, int mc,
                                                      int m, double* __restrict__ h)
{
   __shared__ double s_sum[16][64];
   const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
   const int i = blockIdx.x * 64 + lane;
   const int ii = i < mc ? i : mc - 1;
   double z[4] = {0.0, 0.0, 0.0, 0.0};
   int u = 0;
   for (int b = g; b < nblk; b += 16, u = (u + 1) & 3) z[u] += part[(size_t)b * ldp + ii];
   s_sum[g][lane] = (z[0] + z[1]) + (z[2] + z[3]);
   __syncthreads();
   if (g == 0 && i < mc) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < 16; q++) t += s_sum[q][lane];
      h[i < m ? i : m + 1] = t;
   }
}

// w -= sum_{j < m} h[j] Z[j n + .] (j in order, four columns' loads in flight per step), then *out = ||w||^2
// (fixed-order grid reduction).  c_after / c_before (optional device scalars, the squared norms after and
// before the previous pass): the pass runs only when the DGKS test sqrt(after) < 0.7071 sqrt(before) holds --
// the same in every workgroup -- and *c_flag records the decision (1 / 0) for the host
// VEC = 2: two consecutive rows per 16-byte load (n even, w and Z 16-byte aligned); w's rows get the same bits,
// only the norm's summation order differs
template <int VEC = 1>
__global__ __launch_bounds__(kKThreads) void k_block_update(double* __restrict__ w, const double* __restrict__ Z,
                                                            size_t n, const double* __restrict__ h, int m,
                                                            double* __restrict__ part,
                                                            unsigned int* __restrict__ ticket,
                                                            double* __restrict__ out,
                                                            const double* __restrict__ c_after = nullptr,
                                                            const double* __restrict__ c_before = nullptr,
                                                            double* __restrict__ c_flag = nullptr)
{
   if (c_after) {
      const bool again = sqrt(*c_after) < 0.7071 * sqrt(*c_before);
      if (blockIdx.x == 0 && threadIdx.x == 0) *c_flag = again ? 1.0 : 0.0;
      if (!again) return;
   }
   extern __shared__ double s_h[];
   for (int j = threadIdx.x; j < m; j += kKThreads) s_h[j] = h[j];
   __syncthreads();
   double acc = 0.0;
   if constexpr (VEC == 2) {
      constexpr int E2 = kKEPT / 2;  // pairs per thread per step
      const size_t n2 = n / 2;
      double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
      const size_t stride2 = (size_t)gridDim.x * kKThreads * E2;
      for (size_t p0 = (size_t)blockIdx.x * kKThreads * E2 + threadIdx.x; p0 < n2; p0 += stride2) {
         double2 wv[E2];
         bool in[E2];
#pragma unroll
         for (int e = 0; e < E2; e++) {
            const size_t p = p0 + (size_t)e * kKThreads;
            in[e] = p < n2;
            wv[e] = in[e] ? w2[p] : make_double2(0.0, 0.0);
         }
         int j = 0;
         for (; j + 4 <= m; j += 4) {
            double2 z[4][E2];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
               for (int e = 0; e < E2; e++)
                  z[q][e] = in[e] ? reinterpret_cast<const double2*>(Z + (size_t)(j + q) * n)[p0 + (size_t)e * kKThreads]
                                  : make_double2(0.0, 0.0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
               const double hj = s_h[j + q];
#pragma unroll
               for (int e = 0; e < E2; e++) {
                  wv[e].x = fma(-hj, z[q][e].x, wv[e].x);
                  wv[e].y = fma(-hj, z[q][e].y, wv[e].y);
               }
            }
         }
         for (; j < m; j++) {
            const double hj = s_h[j];
#pragma unroll
            for (int e = 0; e < E2; e++) {
               const double2 z = in[e] ? reinterpret_cast<const double2*>(Z + (size_t)j * n)[p0 + (size_t)e * kKThreads]
                                       : make_double2(0.0, 0.0);
               wv[e].x = fma(-hj, z.x, wv[e].x);
               wv[e].y = fma(-hj, z.y, wv[e].y);
            }
         }
#pragma unroll
         for (int e = 0; e < E2; e++) {
            if (in[e]) w2[p0 + (size_t)e * kKThreads] = wv[e];
            acc = fma(wv[e].y, wv[e].y, fma(wv[e].x, wv[e].x, acc));
         }
      }
      acc = block_sum0<kKThreads>(acc);
      double tot;
      if (grid_total<kKThreads>(acc, part, ticket, &tot) && threadIdx.x == 0) *out = tot;
      return;
   }
   const size_t stride = (size_t)gridDim.x * kKThreads * kKEPT;
   for (size_t i0 = (size_t)blockIdx.x * kKThreads * kKEPT + threadIdx.x; i0 < n; i0 += stride) {
      double wv[kKEPT];
      bool in[kKEPT];
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         const size_t i = i0 + (size_t)e * kKThreads;
         in[e] = i < n;
         wv[e] = in[e] ? w[i] : 0.0;
      }
      int j = 0;
      for (; j + 4 <= m; j += 4) {
         double z[4][kKEPT];
#pragma unroll
         for (int q = 0; q < 4; q++)
#pragma unroll
            for (int e = 0; e < kKEPT; e++) z[q][e] = in[e] ? Z[(size_t)(j + q) * n + i0 + (size_t)e * kKThreads] : 0.0;
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const double hj = s_h[j + q];
#pragma unroll
            for (int e = 0; e < kKEPT; e++) wv[e] = fma(-hj, z[q][e], wv[e]);
         }
      }
      for (; j < m; j++) {
         const double hj = s_h[j];
#pragma unroll
         for (int e = 0; e < kKEPT; e++)
            wv[e] = fma(-hj, in[e] ? Z[(size_t)j * n + i0 + (size_t)e * kKThreads] : 0.0, wv[e]);
      }
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         const size_t i = i0 + (size_t)e * kKThreads;
         if (i < n) w[i] = wv[e];
         acc = fma(wv[e], wv[e], acc);
      }
   }
   acc = block_sum0<kKThreads>(acc);
   double tot;
   if (grid_total<kKThreads>(acc, part, ticket, &tot) && threadIdx.x == 0) *out = tot;
}

// ---- DCGS2 (delayed classical Gram-Schmidt with re-orthogonalisation; FGMRES ortho 2) ----------------------
// Sweep 1 of a step: S[k] = (v_k, a) and T[k] = (v_k, b) for the m basis columns (the last of them is a itself,
// the step's provisional column) -- the previous column's second pass and this column's first pass read the
// basis once together.  Partials: part[blk ldp + k] (S), part[blk ldp + m + k] (T); b may be null.
constexpr int kBD2 = 16;
__global__ __launch_bounds__(kBDThreads) void k_block_dots_ab(const double* __restrict__ a, const double* __restrict__ b,
                                                              const double* __restrict__ V, size_t n, int m,
                                                              double* __restrict__ part, int ldp)
{
   __shared__ double s[kBDThreads / 64][2 * kBD2];
   const int g0 = blockIdx.y * kBD2;
   const int cnt = min(kBD2, m - g0);
   double sa[kBD2], sb[kBD2];
#pragma unroll
   for (int j = 0; j < kBD2; j++) sa[j] = sb[j] = 0.0;
   const size_t stride = (size_t)gridDim.x * kBDThreads;
   for (size_t r = (size_t)blockIdx.x * kBDThreads + threadIdx.x; r < n; r += stride) {
      const double ar = a[r];
      const double br = b ? b[r] : 0.0;
      double v[kBD2];
#pragma unroll
      for (int j = 0; j < kBD2; j++) v[j] = j < cnt ? V[(size_t)(g0 + j) * n + r] : 0.0;
#pragma unroll
      for (int j = 0; j < kBD2; j++) {
         sa[j] = fma(v[j], ar, sa[j]);
         sb[j] = fma(v[j], br, sb[j]);
      }
   }
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
   for (int j = 0; j < kBD2; j++) {
      double x = sa[j], y = sb[j];
      for (int off = 32; off > 0; off >>= 1) {
         x += __shfl_down(x, off, 64);
         y += __shfl_down(y, off, 64);
      }
      if (lane == 0) {
         s[wave][j] = x;
         s[wave][kBD2 + j] = y;
      }
   }
   __syncthreads();
   if (threadIdx.x < 2 * kBD2) {
      const int j = threadIdx.x % kBD2, which = threadIdx.x / kBD2;
      if (j < cnt && (which == 0 || b)) {
         double t = 0.0;
#pragma unroll
         for (int q = 0; q < kBDThreads / 64; q++) t += s[q][threadIdx.x];
         part[(size_t)blockIdx.x * ldp + which * m + g0 + j] = t;
      }
   }
}

// Update of a step (row-parallel, basis columns read once): column j is finalised in place,
// v_j = (V[:, j] - sum_{k<j} s_k v_k) / alpha, and w becomes the next provisional column's numerator
// u = w / alpha - sum_{k<j} g_k v_k - g_j v_j; *out = ||u||^2.  coef = [s (j) | g (j + 1) | 1 / alpha].
__global__ __launch_bounds__(kKThreads) void k_dcgs2_update(double* __restrict__ V, double* __restrict__ w, size_t n,
                                                            int j, const double* __restrict__ coef,
                                                            double* __restrict__ part,
                                                            unsigned int* __restrict__ ticket,
                                                            double* __restrict__ out)
{
   extern __shared__ double s_c[];
   for (int k = threadIdx.x; k < 2 * j + 2; k += kKThreads) s_c[k] = coef[k];
   __syncthreads();
   const double* s_s = s_c;
   const double* s_g = s_c + j;
   const double ia = s_c[2 * j + 1];
   double acc = 0.0;
   const size_t stride = (size_t)gridDim.x * kKThreads * kKEPT;
   double* vjcol = V + (size_t)j * n;
   for (size_t i0 = (size_t)blockIdx.x * kKThreads * kKEPT + threadIdx.x; i0 < n; i0 += stride) {
      double v0[kKEPT], u[kKEPT];
      bool in[kKEPT];
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         const size_t i = i0 + (size_t)e * kKThreads;
         in[e] = i < n;
         v0[e] = in[e] ? vjcol[i] : 0.0;
         u[e] = in[e] ? w[i] * ia : 0.0;
      }
      int k = 0;
      for (; k + 4 <= j; k += 4) {
         double z[4][kKEPT];
#pragma unroll
         for (int q = 0; q < 4; q++)
#pragma unroll
            for (int e = 0; e < kKEPT; e++) z[q][e] = in[e] ? V[(size_t)(k + q) * n + i0 + (size_t)e * kKThreads] : 0.0;
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const double sk = s_s[k + q], gk = s_g[k + q];
#pragma unroll
            for (int e = 0; e < kKEPT; e++) {
               v0[e] = fma(-sk, z[q][e], v0[e]);
               u[e] = fma(-gk, z[q][e], u[e]);
            }
         }
      }
      for (; k < j; k++) {
         const double sk = s_s[k], gk = s_g[k];
#pragma unroll
         for (int e = 0; e < kKEPT; e++) {
            const double z = in[e] ? V[(size_t)k * n + i0 + (size_t)e * kKThreads] : 0.0;
            v0[e] = fma(-sk, z, v0[e]);
            u[e] = fma(-gk, z, u[e]);
         }
      }
      const double gj = s_g[j];
#pragma unroll
      for (int e = 0; e < kKEPT; e++) {
         const size_t i = i0 + (size_t)e * kKThreads;
         const double vj = v0[e] * ia;
         u[e] = fma(-gj, vj, u[e]);
         if (in[e]) {
            vjcol[i] = vj;
            w[i] = u[e];
         }
         acc = fma(u[e], u[e], acc);
      }
   }
   acc = block_sum0<kKThreads>(acc);
   double tot;
   if (grid_total<kKThreads>(acc, part, ticket, &tot) && threadIdx.x == 0) *out = tot;
}

// a *= 1 / sqrt(*nrm2) (the provisional column's normalisation, without a host round trip).  A lucky breakdown
// (u = 0 exactly, e.g. A = I) leaves the zero column as it is: 1 / sqrt(0) would fill it with NaN, and the host
// finishes the Hessenberg column with H(j, j-1) = 0 (convergence)
__global__ void k_scale_rnorm(double* __restrict__ a, size_t n, const double* __restrict__ nrm2)
{
   const double f = *nrm2 > 0.0 ? 1.0 / sqrt(*nrm2) : 0.0;
   for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] *= f;
}

int egrid(size_t n)
{
   size_t g = (n + 255) / 256;
   return (int)std::max<size_t>(1, std::min<size_t>(g, 4096));
}

// device scratch of the Krylov solvers: two reduction pairs, device scalars, pinned read-back
struct KScratch {
   static constexpr int kScal = Ctx::kScal;
   double *part = nullptr, *part2 = nullptr, *scal = nullptr, *hscal = nullptr, *coef = nullptr;
   double* hcoef = nullptr;  // pinned staging of per-step coefficients (DCGS2)
   double* bpart = nullptr;  // block Gram-Schmidt partials [kBDMaxBlocks][kScal]
   unsigned int *ticket = nullptr, *ticket2 = nullptr;
   double* lz_part = nullptr;          // k_lanczos_local: 4 partial arrays
   unsigned int* lz_ticket = nullptr;  // k_lanczos_local: 3 ticket arrays
   int lz_occ = -1;                    // resident k_lanczos_local workgroups
   int* chain = nullptr;      // k_mgs_chain: [1] error word
   int* hchain_err = nullptr; // pinned read-back of the error word
   int chain_occ = -1;        // resident workgroups of k_mgs_chain per CU x CUs (0: unusable)
   int wide_occ[6] = {-1, -1, -1, -1, -1, -1};  // the same for k_mgs_wide<1024, kWideS[x]>
   // set once a one-launch sweep's wait has given up in this process: the sweeps then run as launch chains
   // (k_gs_step / block_gs), which cannot wait on other workgroups
   bool chain_off = false;
   // after a wait gave up: clear the error word and every ticket array the one-launch kernels count on, so
   // later reductions start from zero, and stop using those kernels (chain_off)
   void chain_reset()
   {
      (void)hipDeviceSynchronize();
      if (chain) (void)hipMemset(chain, 0, sizeof(int) * 2);
      if (ticket) (void)hipMemset(ticket, 0, sizeof(unsigned int) * kTicketWords);
      if (lz_ticket) (void)hipMemset(lz_ticket, 0, sizeof(unsigned int) * 3 * kTicketWords);
      if (hchain_err) *hchain_err = 0;
      chain_off = true;
   }
   unsigned int* bd_tickets = nullptr;  // k_block_dots<true>: one ticket array per column group
   int ensure_bpart()
   {
      if (!bpart) NFFT4GP_HIP_CHECK(hipMalloc((void**)&bpart, sizeof(double) * kBDMaxBlocks * kScal));
      if (!bd_tickets) {
         const size_t words = (size_t)(kScal / kBD + 1) * kTicketWords;
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&bd_tickets, sizeof(unsigned int) * words));
         NFFT4GP_HIP_CHECK(hipMemset(bd_tickets, 0, sizeof(unsigned int) * words));
      }
      return 0;
   }
   int ensure()
   {
      if (part) return 0;
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&part, sizeof(double) * kKMaxBlocks));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&part2, sizeof(double) * kKMaxBlocks));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&scal, sizeof(double) * kScal));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&coef, sizeof(double) * kScal));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&ticket, sizeof(unsigned int) * kTicketWords));
      NFFT4GP_HIP_CHECK(hipMalloc((void**)&ticket2, sizeof(unsigned int) * kTicketWords));
      NFFT4GP_HIP_CHECK(hipMemset(ticket, 0, sizeof(unsigned int) * kTicketWords));
      NFFT4GP_HIP_CHECK(hipMemset(ticket2, 0, sizeof(unsigned int) * kTicketWords));
      NFFT4GP_HIP_CHECK(hipHostMalloc((void**)&hscal, sizeof(double) * kScal));
      NFFT4GP_HIP_CHECK(hipHostMalloc((void**)&hcoef, sizeof(double) * kScal));
      return 0;
   }
   int ensure_chain()
   {
      if (ensure()) return -1;
      if (!chain) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&chain, sizeof(int) * 2));
         NFFT4GP_HIP_CHECK(hipMemset(chain, 0, sizeof(int) * 2));
         NFFT4GP_HIP_CHECK(hipHostMalloc((void**)&hchain_err, sizeof(int)));
         *hchain_err = 0;
      }
      if (!lz_part) {
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&lz_part, sizeof(double) * 4 * kKMaxBlocks));
         NFFT4GP_HIP_CHECK(hipMalloc((void**)&lz_ticket, sizeof(unsigned int) * 3 * kTicketWords));
         NFFT4GP_HIP_CHECK(hipMemset(lz_ticket, 0, sizeof(unsigned int) * 3 * kTicketWords));
      }
      if (lz_occ < 0) lz_occ = resident_workgroups(k_lanczos_local<1024, 4>);
      if (chain_occ < 0) {
         chain_occ = resident_workgroups(k_mgs_chain<1024, 4>);
         for (int x = 0; x < 6; x++) wide_occ[x] = resident_workgroups(mgs_wide_fn(kWideS[x]));
      }
      return 0;
   }
};
KScratch g_k;

}  // namespace

namespace {

// the instantiations of the block passes by switch
auto block_dots_fn(bool fold, bool vec)
{
   return fold ? (vec ? k_block_dots<true, 2> : k_block_dots<true, 1>)
               : (vec ? k_block_dots<false, 2> : k_block_dots<false, 1>);
}
auto block_update_fn(bool vec) { return vec ? k_block_update<2> : k_block_update<1>; }

}  // namespace

namespace nfft4gp_amd {

Ctx::Ctx(hipStream_t s_, size_t n_, Comm* comm_) : s(s_), n(n_), comm(comm_)
{
   auto on = [](const char* name) {  // a switch that only "=0" turns off
      const char* e = getenv(name);
      return !(e && atoi(e) == 0);
   };
   chain_on = on("NFFT4GP_AMD_MGS_CHAIN");
   local_on = on("NFFT4GP_AMD_LANCZOS_LOCAL");
   fold_on = on("NFFT4GP_AMD_BD_FOLD");
   vec_on = on("NFFT4GP_AMD_BD_VEC");
   const char* e = getenv("NFFT4GP_AMD_MGS_WIDE");
   wide_set = e != nullptr;
   wide = e ? atoi(e) : 0;
}

double* Ctx::scal(int off) const { return g_k.scal + off; }

int Ctx::mgs_form(unsigned* grid)
{
   *grid = gs_grid(n);
   if (comm || g_k.ensure_chain()) return -1;
   // NFFT4GP_AMD_MGS_WIDE=S (one of kWideS): that S at any n its resident grid covers in S passes, ahead of
   // k_mgs_chain (the tests run every instantiation at small n this way)
   for (int x = 0; x < 6; x++)
      if (wide == kWideS[x]) {
         const size_t per = (size_t)kWideS[x] * 4096;
         const size_t g = (n + per - 1) / per;
         if (g >= 1 && g <= (size_t)g_k.wide_occ[x] && g <= (size_t)kKMaxBlocks) {
            *grid = (unsigned)g;
            return kWideS[x];
         }
      }
   if ((size_t)*grid * 4096 >= n && (int)*grid <= g_k.chain_occ) return 0;
   if (wide_set && wide == 0) return -1;
   for (int x = 0; x < 6; x++) {
      const size_t per = (size_t)kWideS[x] * 4096;
      const size_t g = (n + per - 1) / per;
      if (g <= (size_t)g_k.wide_occ[x] && g <= (size_t)kKMaxBlocks) {
         *grid = (unsigned)g;
         return kWideS[x];
      }
   }
   return -1;
}

int Ctx::gs(double* w, const double* u, const double* hprev, const double* v, double* out, unsigned grid_in)
{
   // 1024 threads x 4 elements: a quarter of the 256-thread partials for the last block to add (8.35 us per
   // projection at n = 1e6 against 9.16; 1024 x 8: 10.7, 512 x 4: 8.49 -- round 3, tools/ab_gs.sh, removed)
   const unsigned grid = grid_in ? grid_in : gs_grid(n);
   hipLaunchKernelGGL((k_gs_step<1024, 4>), dim3(grid), dim3(1024), 0, s, w, u, hprev, v, n, g_k.part, g_k.ticket,
                      out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return red(out, 1);
}

int Ctx::gs_chain(double* w, const double* V, int i, double* hd)
{
   unsigned mg = 0;
   if (mgs_form(&mg) < 0) mg = 0;
   for (int j = 0; j < i; j++)
      if (gs(w, j ? V + (size_t)(j - 1) * n : nullptr, j ? hd + j - 1 : nullptr, V + (size_t)j * n, hd + j, mg))
         return -1;
   return gs(w, i ? V + (size_t)(i - 1) * n : nullptr, i ? hd + i - 1 : nullptr, nullptr, hd + i, mg);
}

int Ctx::mgs_chain(double* w, const double* V, int i, double* hd)
{
   if (comm || g_k.ensure_chain()) return comm ? 1 : -1;
   unsigned grid = 0;
   const int form = mgs_form(&grid);
   if (!chain_on || g_k.chain_off || form < 0) return 1;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(hd, 0xFF, sizeof(double) * (i + 1), s));  // kChainUnset
   if (form > 0)
      hipLaunchKernelGGL(mgs_wide_fn(form), dim3(grid), dim3(1024), 0, s, w, V, n, i, hd, g_k.part, g_k.ticket,
                         g_k.chain + 1);
   else
      hipLaunchKernelGGL((k_mgs_chain<1024, 4>), dim3(grid), dim3(1024), 0, s, w, V, n, i, hd, g_k.part,
                         g_k.ticket, g_k.chain + 1);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   // the error word comes back with the step's scalars (the caller's read synchronises)
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(g_k.hchain_err, g_k.chain + 1, sizeof(int), hipMemcpyDeviceToHost, s));
   return 0;
}

int Ctx::lanczos_local(double* w, const double* Vl, const double* Zl, int ml, double* h)
{
   const unsigned grid = gs_grid(n);
   lz_launched = false;
   if (comm || !local_on || ml < 1 || ml > 2 || g_k.ensure_chain() || (size_t)grid * 4096 < n ||
       (int)grid > g_k.lz_occ || g_k.chain_off)
      return block_gs(w, Vl, Zl, ml, h, 1);
   lz_launched = true;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(h, 0xFF, sizeof(double) * (ml + 2), s));  // kChainUnset
   hipLaunchKernelGGL((k_lanczos_local<1024, 4>), dim3(grid), dim3(1024), 0, s, w, Vl, Zl, Zl == Vl ? 1 : 0, n,
                      ml, h, g_k.lz_part, g_k.lz_ticket, g_k.chain + 1);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(g_k.hchain_err, g_k.chain + 1, sizeof(int), hipMemcpyDeviceToHost, s));
   return 0;
}

int Ctx::chain_failed()
{
   if (*g_k.hchain_err) {
      fprintf(stderr, "nfft4gp_amd: FGMRES: the one-launch MGS sweep's wait gave up\n");
      g_k.chain_reset();
      return 1;
   }
   return 0;
}

int Ctx::lanczos_local_failed()
{
   if (lz_launched && *g_k.hchain_err) {
      fprintf(stderr, "nfft4gp_amd: Lanczos: the one-launch local pass's wait gave up\n");
      g_k.chain_reset();
      return 1;
   }
   return 0;
}

int Ctx::read(const double* d, int count, double* h)
{
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(g_k.hscal, d, sizeof(double) * count, hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   memcpy(h, g_k.hscal, sizeof(double) * count);
   return 0;
}

double Ctx::dot(const double* a, const double* b)
{
   if (gs(const_cast<double*>(a), nullptr, nullptr, b, g_k.scal + KScratch::kScal - 1)) return NAN;
   double v;
   if (read(g_k.scal + KScratch::kScal - 1, 1, &v)) return NAN;
   return v;
}

double Ctx::norm(const double* a) { return std::sqrt(dot(a, a)); }

int Ctx::dot2(const double* v, const double* z, double* out)
{
   hipLaunchKernelGGL(k_dot2, dim3(kgrid(n)), dim3(kKThreads), 0, s, v, z, n, g_k.part, g_k.ticket, g_k.part2,
                      g_k.ticket2, out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return red(out, 2);
}

bool Ctx::bd_vec(const void* a, const void* b, const void* c2) const
{
   return vec_on && n % 2 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c2) & 15) == 0;
}

void Ctx::block_dots(const double* w, const double* V, int m, int with_norm, double* h, bool vec, const double* after,
                     const double* before)
{
   const int nb = bd_grid(n);
   const int mc = m + with_norm;
   hipLaunchKernelGGL(block_dots_fn(fold_on, vec), dim3(nb, (mc + kBD - 1) / kBD), dim3(kBDThreads), 0, s, w, V, n, m,
                      with_norm, g_k.bpart, KScratch::kScal, after, before, fold_on ? h : (double*)nullptr,
                      fold_on ? g_k.bd_tickets : (unsigned int*)nullptr);
   if (!fold_on)
      hipLaunchKernelGGL(k_block_reduce, dim3((mc + 63) / 64), dim3(1024), 0, s, g_k.bpart, nb, KScratch::kScal, mc, m,
                         h);
}

void Ctx::block_update(double* w, const double* Z, int m, const double* h, double* out, bool vec, const double* after,
                       const double* before, double* flag)
{
   hipLaunchKernelGGL(block_update_fn(vec), dim3(kgrid(n)), dim3(kKThreads), sizeof(double) * m, s, w, Z, n, h, m,
                      g_k.part, g_k.ticket, out, after, before, flag);
}

int Ctx::block_gs(double* w, const double* V, const double* Z, int m, double* h, int with_norm)
{
   if (m <= 0 || m + 2 > KScratch::kScal) return -1;
   if (g_k.ensure_bpart()) return -1;
   const bool vec = bd_vec(w, V, Z);
   // h[m], h[m + 1] take part in the all-reduce below even when this pass does not write them
   if (comm) NFFT4GP_HIP_CHECK(hipMemsetAsync(h + m, 0, sizeof(double) * 2, s));
   block_dots(w, V, m, with_norm, h, vec);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (red(h, m + 2)) return -1;  // the projections and the norm before them, summed over the row shards
   block_update(w, Z, m, h, h + m, vec);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return red(h + m, 1);
}

int Ctx::block_cgs2(double* w, const double* V, int m, double* h)
{
   if (m <= 0 || 2 * m + 4 > KScratch::kScal) return -1;
   if (block_gs(w, V, V, m, h, 1)) return -1;
   const bool vec = bd_vec(w, V, V);
   const double* after = h + m;
   const double* before = h + m + 1;
   block_dots(w, V, m, 0, h + m + 2, vec, after, before);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (red(h + m + 2, m)) return -1;
   block_update(w, V, m, h + m + 2, h + 2 * m + 2, vec, after, before, h + 2 * m + 3);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return red(h + 2 * m + 2, 1);
}

int Ctx::dots_ab(const double* a, const double* b, const double* V, int m, double* out)
{
   if (m <= 0 || 2 * m > KScratch::kScal) return -1;
   if (g_k.ensure_bpart()) return -1;
   const int nb = bd_grid(n);
   hipLaunchKernelGGL(k_block_dots_ab, dim3(nb, (m + kBD2 - 1) / kBD2), dim3(kBDThreads), 0, s, a, b, V, n, m,
                      g_k.bpart, KScratch::kScal);
   const int mc = b ? 2 * m : m;
   hipLaunchKernelGGL(k_block_reduce, dim3((mc + 63) / 64), dim3(1024), 0, s, g_k.bpart, nb, KScratch::kScal, mc,
                      mc, out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return red(out, mc);
}

int Ctx::dcgs2_update(double* V, double* w, int j, const std::vector<double>& coef, double* nrm2)
{
   if (coef.size() > (size_t)KScratch::kScal) return -1;
   // pinned staging: the previous step's copy has run (the host read this step's sweep after it)
   memcpy(g_k.hcoef, coef.data(), sizeof(double) * coef.size());
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(g_k.coef, g_k.hcoef, sizeof(double) * coef.size(), hipMemcpyHostToDevice, s));
   hipLaunchKernelGGL(k_dcgs2_update, dim3(kgrid(n)), dim3(kKThreads), sizeof(double) * (2 * j + 2), s, V, w, n, j,
                      g_k.coef, g_k.part, g_k.ticket, nrm2);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   if (red(nrm2, 1)) return -1;
   hipLaunchKernelGGL(k_scale_rnorm, dim3(egrid(n)), dim3(256), 0, s, w, n, (const double*)nrm2);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

void Ctx::scale(double* a, double* b, double f)
{
   hipLaunchKernelGGL(k_scale2, dim3(egrid(n)), dim3(256), 0, s, a, b, n, f);
}

int Ctx::combine(double* x, const double* B, int m, const double* c)
{
   if (m <= 0) return 0;
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(g_k.coef, c, sizeof(double) * m, hipMemcpyHostToDevice, s));
   hipLaunchKernelGGL(k_combine, dim3(egrid(n)), dim3(256), 0, s, x, B, n, n, g_k.coef, m);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int Ctx::sub(double* y, const double* a, const double* b)
{
   hipLaunchKernelGGL(k_sub, dim3(egrid(n)), dim3(256), 0, s, y, a, b, n);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int Ctx::copy(double* dst, const double* src)
{
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
   return 0;
}

// ---- the lockstep batch -------------------------------------------------------------------------------------------
int BatchCtx::pin_wait()
{
   NFFT4GP_HIP_CHECK(hipEventSynchronize(pin_ev.e));
   return 0;
}

int BatchCtx::pin_done()
{
   NFFT4GP_HIP_CHECK(hipEventRecord(pin_ev.e, c.s));
   return 0;
}

int BatchCtx::init(int m_, int kcyc, int colcap_)
{
   m = m_;
   colcap = colcap_;
   if (part.alloc((size_t)m * kKMaxBlocks) || ticket.alloc((size_t)m * kTicketWords) || dact.alloc(m) || pact.alloc(m))
      return -1;
   if (kcyc > 0) {
      if (dfac.alloc(m) || dcoef.alloc((size_t)kcyc) || dcols.alloc((size_t)kcyc) || pin.alloc(4 * m + 2 * kcyc + 16) ||
          dvcols.alloc((size_t)colcap) || derr.alloc(1) || pvcols.alloc(64) || herr.alloc(1))
         return -1;
      *herr = 0;
      NFFT4GP_HIP_CHECK(hipMemsetAsync(derr, 0, sizeof(int), c.s));
   }
   NFFT4GP_HIP_CHECK(hipEventCreateWithFlags(&pin_ev.e, hipEventDisableTiming));
   if (pin_done()) return -1;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(unsigned int) * (size_t)m * kTicketWords, c.s));
   return 0;
}

int BatchCtx::set_active(const std::vector<int>& act)
{
   if (pin_wait()) return -1;
   nact = (int)act.size();
   memcpy(pact, act.data(), sizeof(int) * act.size());
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(dact, pact, sizeof(int) * act.size(), hipMemcpyHostToDevice, c.s));
   return pin_done();
}

int BatchCtx::gs(double* w, size_t ldw, const double* u, size_t ldu, const double* hprev, const double* v, size_t ldv,
                 double* out)
{
   hipLaunchKernelGGL((k_gs_batch<1024, 4>), dim3(gs_grid(c.n), (unsigned)nact), dim3(1024), 0, c.s, w, ldw, u, ldu,
                      hprev, v, ldv, c.n, (const int*)dact, (double*)part, (unsigned int*)ticket, out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int BatchCtx::dot(const double* a, size_t lda, const double* b, size_t ldb, double* out, int count)
{
   hipLaunchKernelGGL((k_gs_batch<1024, 4>), dim3(gs_grid(c.n), (unsigned)count), dim3(1024), 0, c.s,
                      const_cast<double*>(a), lda, (const double*)nullptr, (size_t)0, (const double*)nullptr, b, ldb, c.n,
                      (const int*)dact, (double*)part, (unsigned int*)ticket, out);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

int BatchCtx::scale(double* a, const std::vector<double>& fac)
{
   if (pin_wait()) return -1;
   memcpy(pin, fac.data(), sizeof(double) * m);
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(dfac, pin, sizeof(double) * m, hipMemcpyHostToDevice, c.s));
   if (pin_done()) return -1;
   hipLaunchKernelGGL(k_scale_batch, dim3(std::max(1, egrid(c.n) / std::max(1, nact)), (unsigned)nact), dim3(256), 0, c.s,
                      a, c.n, c.n, (const int*)dact, (const double*)dfac);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

bool BatchCtx::sweep_fits(int i) const
{
   // resident k_mgs_chain<1024, 4, true> workgroups on the device
   static const int occ_batch = resident_workgroups(k_mgs_chain<1024, 4, true>);
   const unsigned grid = gs_grid(c.n);
   return c.chain_on && (size_t)grid * 4096 >= c.n && (long)grid * (long)nact <= (long)occ_batch && i + 1 <= colcap &&
          !*herr;
}

int BatchCtx::sweep(const std::vector<double*>& cols, int i, double* hd)
{
   while (vcols_up <= i) {  // the column table: pointers of columns not uploaded yet
      if (pin_wait()) return -1;
      const int cnt = std::min(64, i + 1 - vcols_up);
      for (int k = 0; k < cnt; k++) pvcols[k] = cols[vcols_up + k];
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(dvcols + vcols_up, pvcols, sizeof(double*) * cnt, hipMemcpyHostToDevice, c.s));
      if (pin_done()) return -1;
      vcols_up += cnt;
   }
   NFFT4GP_HIP_CHECK(hipMemsetAsync(hd, 0xFF, sizeof(double) * (size_t)(i + 1) * m, c.s));  // kChainUnset
   hipLaunchKernelGGL((k_mgs_chain<1024, 4, true>), dim3(gs_grid(c.n), (unsigned)nact), dim3(1024), 0, c.s,
                      (double*)nullptr, (const double*)nullptr, c.n, i, hd, (double*)part, (unsigned int*)ticket,
                      (int*)derr, (const double* const*)dvcols, (const int*)dact, m);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(herr, derr, sizeof(int), hipMemcpyDeviceToHost, c.s));
   return 0;
}

bool BatchCtx::sweep_failed() const { return *herr != 0; }

int BatchCtx::combine_cols(double* x, const std::vector<double*>& cols, size_t off, int cnt, const double* coef)
{
   if (cnt <= 0) return 0;
   if (pin_wait()) return -1;
   double* pc = pin + m;
   const double** pp = (const double**)(pin + m + cnt);
   for (int j = 0; j < cnt; j++) {
      pc[j] = coef[j];
      pp[j] = cols[j] + off;
   }
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(dcoef, pc, sizeof(double) * cnt, hipMemcpyHostToDevice, c.s));
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(dcols, pp, sizeof(double*) * cnt, hipMemcpyHostToDevice, c.s));
   if (pin_done()) return -1;
   hipLaunchKernelGGL(k_combine_cols, dim3(egrid(c.n)), dim3(256), 0, c.s, x, (const double* const*)dcols, c.n,
                      (const double*)dcoef, cnt);
   NFFT4GP_HIP_CHECK(hipGetLastError());
   return 0;
}

bool make_callbacks(Callbacks& cb, int n, func_symmatvec matvec, void* mat, func_solve prec, void* pdata)
{
   cb.matvec = matvec;
   cb.mat = mat;
   cb.prec = pdata ? prec : nullptr;  // the reference tests prec_data, not the function (fgmres.c:148)
   cb.pdata = pdata;
   cb.n = (size_t)n;
   cb.mv_dev = g_cb_mode == 1 || (g_cb_mode == -1 && library_operator((const void*)matvec));
   cb.pc_dev = g_cb_mode == 1 || (g_cb_mode == -1 && library_operator((const void*)prec));
   if (bind_dist(cb)) return false;
   return g_k.ensure() == 0;
}

}  // namespace nfft4gp_amd

// Fault injection for tests/test_gpu_krylov.py: mode 1 sets the one-launch kernels' error word (the state a
// wait that gave up leaves) and re-enables them; mode 0 clears it and re-enables them.  Returns whether the
// one-launch sweeps were off (a wait had given up) before the call.
extern "C" int Nfft4GPAmdDebugChainFault(int mode)
{
   if (g_k.ensure_chain()) return -1;
   const int was_off = g_k.chain_off ? 1 : 0;
   (void)hipDeviceSynchronize();
   const int v = mode ? 1 : 0;
   NFFT4GP_HIP_CHECK(hipMemcpy(g_k.chain + 1, &v, sizeof(int), hipMemcpyHostToDevice));
   *g_k.hchain_err = 0;
   g_k.chain_off = false;
   return was_off;
}

// One orthogonalisation sweep through the solvers' own launch code (Ctx, comm == NULL, the library's stream) for
// tests/test_gpu_krylov_kernels.py.  w (n), V, Z (m columns of n): device.  kind:
//   0  the per-projection MGS chain as FGMRES's fallback makes it (Ctx::gs on mgs_form's grid): h_out[0..m]
//   1  Ctx::mgs_chain (k_mgs_chain / k_mgs_wide<S>): h_out[0..m]; returns 1, nothing run, where it declines
//   2  Ctx::block_gs(w, V, Z, m, h, with_norm): h_out[0..m + 1]
//   3  Ctx::block_cgs2(w, V, m, h): h_out[0..2m + 3]
//   4  Ctx::lanczos_local(w, V, Z, m, h): h_out[0..m + 1]
// m = 0 (kinds 0, 1): the norm only.  h_out: host.  info (host, 6 ints): [0] the MGS form (0 k_mgs_chain, S
// k_mgs_wide<S>, -1 per projection), [1] its grid, [2] bd_vec, [3] the folded reduce, [4] k_lanczos_local
// launched, [5] the one-launch kernels' error word as read back (a set word is handled as the solvers do).
extern "C" int Nfft4GPAmdDebugOrthoSweep(int kind, double* w, const double* V, const double* Z, long long n, int m,
                                         int with_norm, double* h_out, int* info)
{
   if (!need_device("Nfft4GPAmdDebugOrthoSweep") || n <= 0 || m < 0 || 2 * m + 4 > KScratch::kScal || !w || !h_out ||
       !info || g_k.ensure_chain())
      return -1;
   Ctx c{current_stream(), (size_t)n, nullptr};
   double* hd = g_k.scal;
   for (int q = 0; q < 6; q++) info[q] = 0;
   int count = 0;
   bool one_launch = false;
   if (kind == 0 || kind == 1) {
      unsigned mg = 0;
      const int form = c.mgs_form(&mg);
      info[0] = form;
      info[1] = (int)mg;
      count = m + 1;
      if (kind == 1) {
         const int rc = c.mgs_chain(w, V, m, hd);
         if (rc) return rc;
         one_launch = true;
      } else {
         info[0] = -1;
         if (c.gs_chain(w, V, m, hd)) return -1;
      }
   } else if (kind == 2) {
      info[2] = c.bd_vec(w, V, Z) ? 1 : 0;
      info[3] = c.fold_on ? 1 : 0;
      count = m + 2;
      if (c.block_gs(w, V, Z, m, hd, with_norm)) return -1;
   } else if (kind == 3) {
      info[2] = c.bd_vec(w, V, V) ? 1 : 0;
      info[3] = c.fold_on ? 1 : 0;
      count = 2 * m + 4;
      if (c.block_cgs2(w, V, m, hd)) return -1;
   } else if (kind == 4) {
      count = m + 2;
      if (c.lanczos_local(w, V, Z, m, hd)) return -1;
      info[4] = c.lz_launched ? 1 : 0;
      one_launch = c.lz_launched;
      if (!c.lz_launched) {
         info[2] = c.bd_vec(w, V, Z) ? 1 : 0;
         info[3] = c.fold_on ? 1 : 0;
      }
   } else {
      return -1;
   }
   if (c.read(hd, count, h_out)) return -1;
   if (one_launch) {
      info[5] = *g_k.hchain_err;
      if (kind == 1 ? c.chain_failed() : c.lanczos_local_failed()) return -2;
   }
   return 0;
}

// Timing probe for tools/reorth_probe.py: `reps` classical Gram-Schmidt passes (Ctx::block_gs, the Lanczos
// re-orthogonalisation's pass) of the device vector w against m device columns V (dots) / Z (updates) on the
// library's stream; *ms = average pass time (hipEvents), h_out (m + 2 doubles, optional) = the last pass's scalars
extern "C" int Nfft4GPAmdDebugBlockGs(double* w, const double* V, const double* Z, long long n, int m, int with_norm,
                                      int reps, float* ms, double* h_out)
{
   if (!need_device("Nfft4GPAmdDebugBlockGs") || n <= 0 || m <= 0 || reps <= 0 || g_k.ensure()) return -1;
   Ctx c{current_stream(), (size_t)n, nullptr};
   hipEvent_t e0, e1;
   NFFT4GP_HIP_CHECK(hipEventCreate(&e0));
   NFFT4GP_HIP_CHECK(hipEventCreate(&e1));
   int rc = c.block_gs(w, V, Z, m, g_k.scal, with_norm);  // warm-up
   NFFT4GP_HIP_CHECK(hipEventRecord(e0, c.s));
   for (int r = 0; r < reps && rc == 0; r++) rc = c.block_gs(w, V, Z, m, g_k.scal, with_norm);
   NFFT4GP_HIP_CHECK(hipEventRecord(e1, c.s));
   NFFT4GP_HIP_CHECK(hipEventSynchronize(e1));
   float t = 0.f;
   NFFT4GP_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
   if (ms) *ms = t / reps;
   (void)hipEventDestroy(e0);
   (void)hipEventDestroy(e1);
   if (rc == 0 && h_out) rc = c.read(g_k.scal, m + 2, h_out);
   return rc;
}
