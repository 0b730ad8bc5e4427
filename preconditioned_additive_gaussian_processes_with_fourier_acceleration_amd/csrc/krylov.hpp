// krylov.hpp -- what the Krylov solvers' files share: Ctx (every launch of a Gram-Schmidt / vector kernel of
// krylov.hip goes through it or through BatchCtx), the owners of device and pinned memory, the solvers' report
// lines, and the drivers' prototypes (fgmres.hip, lanczos.hip; gp_loss.hip calls them).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "callbacks.hpp"
#include "internal.h"

namespace nfft4gp_amd {

inline double* rel_hist(int len)
{
   return (double*)calloc((size_t)std::max(1, len), sizeof(double));
}

template <class T>
int dmalloc(T** p, size_t count)
{
   NFFT4GP_HIP_CHECK(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(1, count)));
   return 0;
}

// owners of a device buffer, a pinned host buffer and an event: freed on every way out of their scope.  Whoever
// holds them synchronises the stream first where work may still read them.
template <class T>
struct DevBuf {
   T* p = nullptr;
   DevBuf() = default;
   DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
   DevBuf(const DevBuf&) = delete;
   DevBuf& operator=(const DevBuf&) = delete;
   ~DevBuf() { (void)hipFree(p); }
   int alloc(size_t count) { return dmalloc(&p, count); }
   operator T*() const { return p; }
};

template <class T>
struct PinBuf {
   T* p = nullptr;
   PinBuf() = default;
   PinBuf(const PinBuf&) = delete;
   PinBuf& operator=(const PinBuf&) = delete;
   ~PinBuf()
   {
      if (p) (void)hipHostFree(p);
   }
   int alloc(size_t count)
   {
      if (hipHostMalloc((void**)&p, sizeof(T) * count) == hipSuccess) return 0;
      p = nullptr;
      return -1;
   }
   operator T*() const { return p; }
};

struct EventHold {
   hipEvent_t e = nullptr;
   EventHold() = default;
   EventHold(const EventHold&) = delete;
   EventHold& operator=(const EventHold&) = delete;
   ~EventHold()
   {
      if (e) (void)hipEventDestroy(e);
   }
};

// declared after the owners whose buffers the stream's queued work may still use: it drains before they are freed
struct SyncOnExit {
   hipStream_t s;
   ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

// closes a Vec (callbacks.hpp) without copying back on every way out of its scope
struct VecClose {
   Vec& v;
   ~VecClose() { (void)v.close(false); }
};

// The report lines of the solvers (the reference's printf calls in fgmres.c and lanczos.c): to stdout, or
// appended to *to (the batch driver prints per system at the end).
struct Report {
   std::string* to = nullptr;
   // the banner, "Start FlexGMRES(kdim)" or "Start Lanczos(maxits)" by name and dim, and the line of step 0
   void header(const char* name, int dim, double tolr, int maxits, double normr, double rel0) const
   {
      const char* rule = "--------------------------------------------------------------------------------\n";
      put("%s", rule);
      put("Start %s(%d)\n", name, dim);
      put("Residual Tol: %e\nMax number of inner iterations: %d\n", tolr, maxits);
      put("%s", rule);
      put("Step    Residual norm  Relative res.  Convergence Rate\n");
      put("%5d   %8e   %8e   N/A\n", 0, normr, rel0);
   }
   void step(int iter, double normr, double rel, double rel_prev) const
   {
      put("%5d   %8e   %8e   %8.6f\n", iter, normr, rel, rel / rel_prev);
   }
   void cycle_end(int kdim, int iter, double rel) const
   {
      put("Rel. residual at the end of current cycle (# of steps per cycle/total its: %d/%d): %e \n", kdim, iter, rel);
   }

private:
   __attribute__((format(printf, 2, 3))) void put(const char* fmt, ...) const
   {
      va_list ap;
      va_start(ap, fmt);
      if (to) {
         char buf[256];
         vsnprintf(buf, sizeof(buf), fmt, ap);
         *to += buf;
      } else {
         vprintf(fmt, ap);
      }
      va_end(ap);
   }
};

// One solve's (or one debug sweep's) way to the device: the stream, the vector length, the row shards' all-reduce
// and the switches, read once when it is made.  Its members launch the kernels of krylov.hip on the library's
// scratch (KScratch there); their scalars land in the device scalar buffer scal(), kScal doubles.
struct Ctx {
   static constexpr int kScal = 4096;
   hipStream_t s;
   size_t n;
   // row-sharded vectors (a distributed operator's rows): every inner product is a local partial, summed
   // in place over the ranks on the stream before anything reads it; NULL for whole vectors
   Comm* comm;
   bool lz_launched = false;  // the last lanczos_local call launched k_lanczos_local
   // the switches (each "=0" turns its form off): NFFT4GP_AMD_MGS_CHAIN the one-launch MGS sweeps,
   // NFFT4GP_AMD_LANCZOS_LOCAL k_lanczos_local, NFFT4GP_AMD_BD_FOLD k_block_reduce folded into k_block_dots,
   // NFFT4GP_AMD_BD_VEC the block passes' 16-byte row pairs; NFFT4GP_AMD_MGS_WIDE=S (wide_set: given) forces
   // k_mgs_wide<1024, S>, 0 leaves k_mgs_wide out
   bool chain_on, local_on, fold_on, vec_on, wide_set;
   int wide;
   Ctx(hipStream_t s, size_t n, Comm* comm = nullptr);

   double* scal(int off = 0) const;  // the device scalar buffer, from entry off
   int red(double* d, int count) { return comm ? comm->allreduce(d, (size_t)count, s) : 0; }
   int read(const double* d, int count, double* h);
   // the MGS sweep's form for this n (comm == NULL): 0 k_mgs_chain (one pass of 4 elements per thread covers n with
   // a resident grid), S > 0 k_mgs_wide<1024, S> on *grid workgroups (the smallest S whose resident grid covers n
   // in S passes), -1 neither (the per-projection chain on its usual grid)
   int mgs_form(unsigned* grid);
   // w -= h u (u optional), *out = (w, v) or ||w||^2; grid 0: the usual grid, else that many workgroups
   // (grid-stride over n: the MGS sweep's grid when k_mgs_wide serves this n, so the two forms are bitwise equal)
   int gs(double* w, const double* u, const double* hprev, const double* v, double* out, unsigned grid = 0);
   // the MGS sweep as one launch per projection (w against V[0..i), then ||w||^2) into hd[0..i], on the grid of
   // the one-launch form this n would take, so the two are bitwise equal; i = 0: the norm only
   int gs_chain(double* w, const double* V, int i, double* hd);
   // the same sweep in one launch when the grid fits (k_mgs_chain / k_mgs_wide); returns 1 when it does not (the
   // caller runs gs_chain).  After the read that follows: chain_failed
   int mgs_chain(double* w, const double* V, int i, double* hd);
   // mgs2's local pass (block_gs(w, Vl, Zl, ml, h, 1)) in one launch where the grid fits (k_lanczos_local);
   // otherwise block_gs.  After the read that follows: lanczos_local_failed
   int lanczos_local(double* w, const double* Vl, const double* Zl, int ml, double* h);
   // did a wait of the last one-launch sweep give up?  Then this solve fails, the error word and the tickets are
   // reset and later sweeps in this process run as launch chains
   int chain_failed();
   int lanczos_local_failed();
   double dot(const double* a, const double* b);
   double norm(const double* a);
   // out[0] = (v, z), out[1] = ||z||^2 (k_dot2), summed over the row shards
   int dot2(const double* v, const double* z, double* out);
   // the block passes' 16-byte row pairs: n even and every vector 16-byte aligned (then so is every column)
   bool bd_vec(const void* a, const void* b, const void* c2) const;
   // h[0..mc) = V^T w (column m, when mc = m + 1, is w itself: h[m + 1]) in k_block_dots (+ k_block_reduce
   // unless folded); after / before: the DGKS gate of a second pass
   void block_dots(const double* w, const double* V, int m, int with_norm, double* h, bool vec,
                   const double* after = nullptr, const double* before = nullptr);
   // w -= Z h (m columns), *out = ||w||^2; after / before / flag: the DGKS gate of a second pass
   void block_update(double* w, const double* Z, int m, const double* h, double* out, bool vec,
                     const double* after = nullptr, const double* before = nullptr, double* flag = nullptr);
   // one classical Gram-Schmidt pass: h[0..m) = V^T w, w -= Z h, h[m] = ||w||^2 afterwards (device
   // scalars); with_norm: also h[m + 1] = ||w||^2 before the update (from the dot pass)
   int block_gs(double* w, const double* V, const double* Z, int m, double* h, int with_norm = 0);
   // CGS2 against the basis V (m columns) with one host read: pass 1 (dots with the norm before, update with
   // the norm after), then pass 2 with every launch gated on the device by the DGKS test on pass 1's norms, so
   // the host does not wait between the passes.  h: [0, m) pass-1 projections, h[m] ||w||^2 after pass 1,
   // h[m + 1] before it, [m + 2, 2m + 2) pass-2 projections, h[2m + 2] ||w||^2 after pass 2, h[2m + 3] the
   // decision (1 / 0); pass-2 entries are meaningful only when the decision is 1
   int block_cgs2(double* w, const double* V, int m, double* h);
   // DCGS2 sweep 1: out[0, m) = V(:, 0..m)^T a, out[m, 2m) = V(:, 0..m)^T b (b optional; column m - 1 is a)
   int dots_ab(const double* a, const double* b, const double* V, int m, double* out);
   // DCGS2 update (k_dcgs2_update) with the host's coefficients [s | g | 1/alpha], then w /= ||w|| on the
   // device; *nrm2 = ||w||^2 before that scaling
   int dcgs2_update(double* V, double* w, int j, const std::vector<double>& coef, double* nrm2);
   void scale(double* a, double* b, double f);                  // a *= f, b *= f (b optional)
   int combine(double* x, const double* B, int m, const double* c);  // x += sum_j c[j] B[:, j]
   int sub(double* y, const double* a, const double* b);        // y = a - b
   int copy(double* dst, const double* src);
};

// The launches of a batch of m systems in lockstep (fgmres_batch_dev, and the predict's dots): Ctx's kernels with
// blockIdx.y over the running systems, on partials, tickets and an error word of its own (one pair per system).
struct BatchCtx {
   Ctx c;
   int m = 0;
   explicit BatchCtx(hipStream_t s, size_t n) : c(s, n) {}
   // partials, tickets and the running list for m systems; kcyc > 0: also the staging of scale and combine_cols
   // (up to kcyc columns) and the one-launch sweep's column table (colcap columns) and error word
   int init(int m, int kcyc = 0, int colcap = 0);
   int set_active(const std::vector<int>& act);  // stream-ordered: launches already queued still read the old list
   // w_s -= hprev[s] u_s (u optional), out[s] = (w_s, v_s) or ||w_s||^2, for the running systems
   int gs(double* w, size_t ldw, const double* u, size_t ldu, const double* hprev, const double* v, size_t ldv,
          double* out);
   // out[s] = (a_s, b_s) for the first `count` systems of the running list: k_gs_step's dot, batched
   int dot(const double* a, size_t lda, const double* b, size_t ldb, double* out, int count);
   int scale(double* a, const std::vector<double>& fac);  // a_s *= fac[s] for the running systems
   // the MGS sweep of step i (column i of every running system against columns [0, i) of cols, then its norm)
   // into hd[j m + s]: sweep_fits, then sweep, then after the read that follows sweep_failed
   bool sweep_fits(int i) const;
   int sweep(const std::vector<double*>& cols, int i, double* hd);
   bool sweep_failed() const;
   // x += sum_j coef[j] (cols[j] + off), j < cnt
   int combine_cols(double* x, const std::vector<double*>& cols, size_t off, int cnt, const double* coef);

private:
   int nact = 0;
   DevBuf<double> part, dfac, dcoef;
   DevBuf<unsigned int> ticket;
   DevBuf<int> dact, derr;
   DevBuf<const double*> dcols, dvcols;
   PinBuf<double> pin;  // pinned: [0, m) factors, then the combine's coefficients and column pointers
   PinBuf<int> pact, herr;
   PinBuf<const double*> pvcols;  // pinned staging of new column pointers
   int vcols_up = 0, colcap = 0;
   EventHold pin_ev;  // the last copy out of the pinned staging: it is rewritten only after that copy has run
   SyncOnExit sync{c.s};  // (declared after every buffer: the stream drains before they are freed)
   int pin_wait();
   int pin_done();
};

struct BatchOut {
   std::vector<int> iters;
   std::vector<double> rel_res;
};

bool make_callbacks(Callbacks& cb, int n, func_symmatvec matvec, void* mat, func_solve prec, void* pdata);

// fgmres.hip
int fgmres_dev(Callbacks& cb, double* x, const double* rhs, int kdim, int maxits, int atol, double tol,
               double* prel_res, double** prel_res_v, int* piter, int print_level);
int fgmres_batch_dev(Callbacks& cb, int m, double* X, size_t ldx, const double* B, size_t ldb, int kdim, int maxits,
                     int atol, double tol, int print_level, BatchOut& res);
// lanczos.hip
int lanczos_dev(Callbacks& cb, double* x, const double* rhs, int wsize, int maxits, int atol, double tol,
                double* prel_res, double** prel_res_v, int* piter, int* tsize, double** TDp, double** TEp,
                int print_level);
int lanczos_pair_dev(Callbacks& cb, double* const* x, const double* const* rhs, int maxits, int print_level,
                     double* prel_res, int* tsize, double** TD, double** TE);
int lanczos_logdet_dev(Callbacks& cb, Callbacks& dcb, func_trace tracefunc, func_logdet logdetfunc,
                       func_dvp dvpfunc, int maxits, int nvecs, const double* radamacher, int print_level,
                       double* logdet, double** dlogdetp);

}  // namespace nfft4gp_amd
