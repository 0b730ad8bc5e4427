// lanczos.hip -- preconditioned Lanczos on device vectors, two runs in lockstep for the probe pairs, and the
// stochastic Lanczos quadrature of the log-determinant and its derivatives.
//
//   Nfft4GPSolverLanczos           SRC/solvers/lanczos.c:3-419  M-inner-product Lanczos with full MGS2
//                                                               re-orthogonalisation (Nfft4GPModifiedGS2,
//                                                               SRC/linearalg/matops.c:348-440)
//   Nfft4GPLanczosQuadratureLogdet SRC/solvers/lanczos.c:421-610
//
// The Cholesky of T and the tridiagonal eigensolve run on the host on scalars read back once per iteration; every
// vector operation is a member of Ctx (krylov.hpp: the kernels and their launches are krylov.hip's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krylov.hpp"

using namespace nfft4gp_amd;

namespace nfft4gp_amd {

// host tridiagonal eigensolve: dstev 'V' (ascending eigenvalues, eigenvectors in columns of TV)
static int tridiag_eig(int m, const double* d, const double* e, std::vector<double>& w, std::vector<double>& V)
{
   std::vector<double> A((size_t)m * m, 0.0);
   for (int i = 0; i < m; i++) {
      A[(size_t)i * m + i] = d[i];
      if (i + 1 < m) {
         A[(size_t)i * m + i + 1] = e[i];
         A[(size_t)(i + 1) * m + i] = e[i];
      }
   }
   return sym_eig_host(A, m, w, V);
}

// ---- Lanczos (lanczos.c:3-419) on device vectors ----------------------------------------------------
// Re-orthogonalisation of w against V[0..k] (dots) / Z[0..k] (updates), adding the projections on v_{k-1}
// and v_k to te / td (Nfft4GPModifiedGS2, matops.c:348-440: MGS over the whole basis, repeated while ||w||
// drops below 0.7071 of its previous value).  Here:
//   1. a local classical pass against the last one or two basis vectors (v_{k-1}, v_k: the three-term
//      recurrence, where the large projections of a Lanczos step are), with ||w|| before it;
//   2. classical passes over the whole basis (Ctx::block_gs: one launch for all the dots, one for the update),
//      repeated while ||w|| drops below 0.7071 of its value before the pass (the DGKS / "twice is enough"
//      test the reference applies), at least one.
// After the local pass the whole-basis projections are at rounding level, so one whole pass normally ends the
// step: the basis is read twice per step instead of four times (two whole passes, the round-3 scheme).  In
// exact arithmetic the projections equal MGS's; in floating point they differ by rounding.
// the local pass's columns at step k: *ml (1 or 2) basis vectors from v_j0 (v_{k-1}, v_k)
static void local_span(int k, int* j0, int* ml)
{
   *j0 = k >= 1 ? k - 1 : 0;
   *ml = k + 1 - *j0;
}

// 2. above, after a pass that left ||w|| = normw: a whole-basis pass, its scalars read back, its projections on
// v_{k-1} and v_k added to *te / *td, *t = ||w|| after it; again while the DGKS test asks for it
static int whole_passes(Ctx& c, double* w, const double* V, const double* Z, int k, double normw, double* td,
                        double* te, double* t)
{
   double* hd = c.scal();
   std::vector<double> h(k + 2);
   for (;;) {
      if (c.block_gs(w, V, Z, k + 1, hd, 0) || c.read(hd, k + 2, h.data())) return -1;
      if (k >= 1) *te += h[k - 1];
      *td += h[k];
      *t = std::sqrt(h[k + 1]);
      if (!(*t < normw * 0.7071 && *t >= DBL_EPSILON)) break;
      normw = *t;
   }
   return 0;
}

static int mgs2(Ctx& c, double* w, const double* V, const double* Z, int k, double* td, double* te, double* t)
{
   double* hd = c.scal();
   const size_t n = c.n;
   int j0, ml;
   local_span(k, &j0, &ml);
   if (c.block_gs(w, V + (size_t)j0 * n, Z + (size_t)j0 * n, ml, hd, 1)) return -1;
   double hl[4];
   if (c.read(hd, ml + 2, hl)) return -1;
   if (k >= 1) *te = hl[0];
   *td = hl[ml - 1];
   *t = std::sqrt(hl[ml]);          // ||w|| after the local pass
   if (*t < DBL_EPSILON) return 0;  // w lies in span(v_{k-1}, v_k): the reference's loop stops here too
   return whole_passes(c, w, V, Z, k, *t, td, te, t);
}

// One Lanczos run as a resumable object, so that two probes of the quadrature can share their matvecs
// (lanczos_pair_dev).  lanczos_dev drives one run the way lanczos.c does.
struct LanczosRun {
   Callbacks& cb;
   Ctx c;
   size_t n;
   double* x;
   int wsize, maxits, print_level;
   double tol;
   int atol;
   bool alias = false;
   DevBuf<double> Vb, Zb;  // the basis; Zb only when preconditioned (else Z == V)
   double *V = nullptr, *Z = nullptr, *z = nullptr, *v = nullptr, *wv = nullptr;
   double *TD = nullptr, *TE = nullptr, *rel = nullptr;
   double **TDp, **TEp;
   std::vector<double> TLD, TLE, y;
   double normb = 0.0, beta = 0.0, tolr = 0.0, normr = 0.0, ls = 0.0, t = 0.0, dotvz = 0.0;
   int iter = 0, chol_size = 0;
   bool done_early = false;  // the run ended in init (n == 0, b == 0, beta == 0): outputs already set
   static constexpr double EPS = DBL_EPSILON;

   LanczosRun(Callbacks& cb_, double* x_, int wsize_, int maxits_, int atol_, double tol_, int print_level_,
              double** TDp_, double** TEp_)
       : cb(cb_), c{current_stream(), cb_.n, cb_.comm}, n(cb_.n), x(x_), wsize(wsize_), maxits(maxits_),
         print_level(print_level_), tol(tol_), atol(atol_), TDp(TDp_), TEp(TEp_)
   {
      if (wsize <= 0) wsize = maxits;
      wsize = std::min(wsize, maxits);
   }
   ~LanczosRun()
   {
      if (Vb.p || Zb.p) (void)hipStreamSynchronize(c.s);  // (before the owners free the basis)
      if (TD && TD != *TDp) free(TD);
      if (TE && TE != *TEp) free(TE);
      free(rel);
   }
   // everything before the first step; returns -1 on error, 1 when the run is already complete
   int init(const double* rhs, double* prel_res, double** prel_res_v, int* piter)
   {
      if (cb.n_global == 0) {
         *prel_res = 0.0;
         *piter = 0;
         *prel_res_v = rel_hist(1);
         done_early = true;
         return 1;
      }
      normb = c.norm(rhs);
      if (normb < EPS) {
         NFFT4GP_HIP_CHECK(hipMemsetAsync(x, 0, sizeof(double) * n, c.s));
         *prel_res = 0.0;
         *piter = 0;
         *prel_res_v = rel_hist(1);
         done_early = true;
         return 1;
      }
      if (maxits + 2 > Ctx::kScal) {
         fprintf(stderr, "nfft4gp_amd: Nfft4GPSolverLanczos: maxits %d above %d\n", maxits, Ctx::kScal - 2);
         return -1;
      }
      // without a preconditioner v = z at every step (the same copy, scaled by the same factor), so the
      // basis is stored once and is its own update basis
      alias = !cb.prec;
      if (Vb.alloc(n * (size_t)(maxits + 1)) || (!alias && Zb.alloc(n * (size_t)(maxits + 1)))) return -1;
      V = Vb;
      Z = alias ? V : Zb;
      TLD.assign(maxits + 1, 0.0);
      TLE.assign(maxits + 1, 0.0);
      y.assign(maxits + 1, 0.0);
      TD = *TDp ? *TDp : (double*)calloc((size_t)maxits + 1, sizeof(double));
      TE = *TEp ? *TEp : (double*)calloc((size_t)std::max(1, maxits), sizeof(double));
      z = Z;
      v = V;
      c.copy(z, rhs);
      if (cb.apply(-1.0, x, 1.0, z)) return -1;
      if (cb.prec) {
         if (cb.solve(v, z)) return -1;
      } else if (!alias) {
         c.copy(v, z);
      }
      normr = c.norm(z);
      beta = std::sqrt(c.dot(v, z));
      if (beta < EPS) {
         *prel_res = 0.0;
         *piter = 0;
         *prel_res_v = rel_hist(1);
         done_early = true;
         return 1;
      }
      tolr = atol ? tol / beta : tol;
      rel = rel_hist(maxits + 1);
      rel[0] = normr / normb;
      if (print_level > 0) Report{}.header("Lanczos", maxits, tolr, maxits, normr, rel[0]);
      c.scale(v, alias ? nullptr : z, 1.0 / beta);
      return 0;
   }
   // a step up to its matvec: z_iter = A v_{iter-1} is the caller's
   void step_begin()
   {
      iter++;
      z = Z + (size_t)iter * n;
      wv = V + (size_t)(iter - 1) * n;
      v = V + (size_t)iter * n;
   }
   // the rest of the step; 1 ends the loop (breakdown, or convergence in the first loop)
   // the fast step (one host read): k of this step, and whether its scalars fit a region of kRegion doubles
   static constexpr int kB0 = 8;
   static constexpr int kRegion = Ctx::kScal / 2;
   int step_k(bool first_loop) const { return first_loop ? std::min(iter - 1, wsize) : iter - 1; }
   bool fast_ok(bool first_loop) const { return kB0 + step_k(first_loop) + 1 + 4 <= kRegion; }
   int region_len(bool first_loop) const { return kB0 + step_k(first_loop) + 1 + 4; }
   // mgs2's local pass and first whole-basis pass, then (speculatively) the preconditioner and k_dot2 of the
   // step, scalars into hd[0, region_len): the host needs mgs2's scalars only to decide whether a further pass
   // is due (rare after the local pass) or w broke down, and in both cases the speculative results are
   // dropped (a further pass recomputes them; a breakdown restarts v and z).  Same kernels, same order, same
   // values as mgs2 followed by the solve and the dot.
   int step_enqueue(bool first_loop, double* hd)
   {
      const int k = step_k(first_loop);
      const int m = k + 1;
      int j0, ml;
      local_span(k, &j0, &ml);
      if (c.lanczos_local(z, V + (size_t)j0 * n, Z + (size_t)j0 * n, ml, hd)) return -1;
      if (c.block_gs(z, V, Z, m, hd + kB0, 0)) return -1;
      if (cb.prec && cb.solve(v, z)) return -1;
      return c.dot2(v, z, hd + kB0 + m + 2);
   }
   // where this step's projections on v_k and v_{k-1} go (the first step has no v_{k-1}: *dummy)
   double* td_of() const { return TD + iter - 1; }
   double* te_of(double* dummy) const { return iter >= 2 ? TE + iter - 2 : dummy; }
   // the preconditioner and the dot of the step's final w, read back: vz = (v, z), ||z||^2
   int solve_dot2(double* vz)
   {
      if (cb.prec && cb.solve(v, z)) return -1;
      double* o = c.scal(Ctx::kScal - 2);
      if (c.dot2(v, z, o) || c.read(o, 2, vz)) return -1;
      return 0;
   }
   // the host side of step_enqueue's scalars hh (read back): mgs2's bookkeeping and repeat rule, then the step's
   // tail; 1 ends the loop
   int step_after(bool first_loop, const double* hh)
   {
      if (c.lanczos_local_failed()) return -1;
      const int k = step_k(first_loop);
      const int m = k + 1;
      int j0, ml;
      local_span(k, &j0, &ml);
      double te_dummy;
      double* tdp = td_of();
      double* tep = te_of(&te_dummy);
      if (k >= 1) *tep = hh[0];
      *tdp = hh[ml - 1];
      const double normw = std::sqrt(hh[ml]);  // ||w|| after the local pass
      if (normw < DBL_EPSILON) {                // mgs2 stops after the local pass
         t = normw;
         return 1;
      }
      const double* h = hh + kB0;
      if (k >= 1) *tep += h[k - 1];
      *tdp += h[k];
      t = std::sqrt(h[k + 1]);
      double vz[2] = {hh[kB0 + m + 2], hh[kB0 + m + 3]};
      if (t < normw * 0.7071 && t >= DBL_EPSILON) {
         // mgs2's repeat rule, then the solve and the dot of the final w (the speculative ones are dropped)
         if (whole_passes(c, z, V, Z, k, t, tdp, tep, &t)) return -1;
         if (t < EPS) return 1;
         if (solve_dot2(vz)) return -1;
      } else if (t < EPS) {
         return 1;
      }
      return step_tail(first_loop, vz);
   }
   int step_end(bool first_loop)
   {
      if (fast_ok(first_loop)) {
         const int len = region_len(first_loop);
         std::vector<double> hh(len);
         if (step_enqueue(first_loop, c.scal()) || c.read(c.scal(), len, hh.data())) return -1;
         return step_after(first_loop, hh.data());
      }
      double te_dummy, vz[2];
      if (mgs2(c, z, V, Z, step_k(first_loop), td_of(), te_of(&te_dummy), &t)) return -1;
      if (t < EPS) return 1;
      if (solve_dot2(vz)) return -1;
      return step_tail(first_loop, vz);
   }
   // the rest of a step from (v, z) and ||z||^2 (the scaling, the Cholesky of T, the residual estimate)
   int step_tail(bool first_loop, const double* vz)
   {
      dotvz = std::sqrt(vz[0]);
      if (dotvz < EPS) return 1;
      c.scale(v, alias ? nullptr : z, 1.0 / dotvz);
      if (first_loop) {
         const double normz = std::sqrt(vz[1]) / dotvz;
         if (iter != 1) {
            TLE[iter - 2] = TE[iter - 2] / TLD[iter - 2];
            TLD[iter - 1] = std::sqrt(TD[iter - 1] - TLE[iter - 2] * TLE[iter - 2]);
            const double le = 1.0 / TLD[iter - 1];
            ls = -ls * TLE[iter - 2] * le;
            normr = std::fabs(le * ls) * dotvz * beta * normz;
         } else {
            TLD[0] = std::sqrt(TD[0]);
            ls = 1.0 / TLD[0];
            normr = dotvz / TD[0] * beta * normz;
         }
         chol_size++;
         rel[iter] = normr / normb;
         if (print_level > 0) Report{}.step(iter, normr, rel[iter], rel[iter - 1]);
         if (normr <= tolr) return 1;
      } else if (print_level > 0) {
         printf("%5d   Building T\n", iter);
      }
      return 0;
   }
   int step(bool first_loop)
   {
      step_begin();
      if (cb.apply(1.0, wv, 0.0, z)) return -1;
      return step_end(first_loop);
   }
   // after the first loop: the solution from the Cholesky factor of T (lanczos.c:258-273), then the second
   // loop that completes T up to wsize, restarting from a random vector after a breakdown
   int finish(double* prel_res, double** prel_res_v, int* piter, int* tsize)
   {
      if (print_level == 0)
         printf("Rel. residual at the end of the iteration (# of its: %d): %e \n", iter, rel[iter]);
      if (chol_size > 0) {
         y[0] = beta / TLD[0];
         for (int k = 1; k < chol_size; k++) y[k] = (-y[k - 1] * TLE[k - 1]) / TLD[k];
         y[chol_size - 1] /= TLD[chol_size - 1];
         for (int k = chol_size - 2; k >= 0; k--) y[k] = (y[k] - TLE[k] * y[k + 1]) / TLD[k];
         if (c.combine(x, V, chol_size, y.data())) return -1;
      }
      *prel_res = normr / normb;
      *piter = iter;
      *prel_res_v = rel;
      rel = nullptr;
      while (iter < wsize) {
         if (t < EPS || dotvz < EPS) {
            z = Z + (size_t)iter * n;
            v = V + (size_t)iter * n;
            // Nfft4GPVecRand of the whole vector (every rank draws the same n_global numbers; a row shard
            // keeps its rows)
            std::vector<double> rnd(cb.n_global);
            {
               CallerRandBatch caller;
               for (size_t i = 0; i < cb.n_global; i++) rnd[i] = (double)rand() / (double)RAND_MAX;
            }
            NFFT4GP_HIP_CHECK(hipMemcpy(z, rnd.data() + cb.row_begin, sizeof(double) * n, hipMemcpyHostToDevice));
            double td, te;
            if (mgs2(c, z, V, Z, iter - 1, &td, &te, &t)) return -1;
            if (t < EPS) break;
            if (cb.prec) {
               if (cb.solve(v, z)) return -1;
            }
            dotvz = std::sqrt(c.dot(v, z));
            if (dotvz < EPS) break;
            c.scale(v, alias ? nullptr : z, 1.0 / dotvz);
         }
         while (iter < wsize) {
            const int r = step(false);
            if (r < 0) return -1;
            if (r) break;
         }
      }
      *tsize = iter;
      *TDp = TD;
      *TEp = TE;
      return 0;
   }
};

int lanczos_dev(Callbacks& cb, double* x, const double* rhs, int wsize, int maxits, int atol, double tol,
                double* prel_res, double** prel_res_v, int* piter, int* tsize, double** TDp, double** TEp,
                int print_level)
{
   LanczosRun L(cb, x, wsize, maxits, atol, tol, print_level, TDp, TEp);
   const int r0 = L.init(rhs, prel_res, prel_res_v, piter);
   if (r0) return r0 < 0 ? -1 : 0;
   while (L.iter < L.maxits) {
      const int r = L.step(true);
      if (r < 0) return -1;
      if (r) break;
   }
   return L.finish(prel_res, prel_res_v, piter, tsize);
}

// Two quadrature probes' Lanczos runs in lockstep through their first loops: while both run, each step's
// two matvecs are one two-vector matvec (launch pair, Nfft4GPAmdAdditiveMatSymvMulti).  Each run computes
// what lanczos_dev computes (the two-vector kernels sum in a different order: rounding-level
// differences); run 0's finish (and any rand() draws of its restarts) comes before run 1's, as in the
// reference's probe order.
int lanczos_pair_dev(Callbacks& cb, double* const* x, const double* const* rhs, int maxits, int print_level,
                     double* prel_res, int* tsize, double** TD, double** TE)
{
   LanczosRun L0(cb, x[0], maxits, maxits, 0, DBL_EPSILON, print_level, &TD[0], &TE[0]);
   LanczosRun L1(cb, x[1], maxits, maxits, 0, DBL_EPSILON, print_level, &TD[1], &TE[1]);
   LanczosRun* R[2] = {&L0, &L1};
   double* relv[2] = {nullptr, nullptr};
   int piter[2] = {0, 0};
   int st[2];  // 0 running the first loop, 1 first loop over, 2 complete in init
   for (int k = 0; k < 2; k++) {
      const int r = R[k]->init(rhs[k], &prel_res[k], &relv[k], &piter[k]);
      if (r < 0) return -1;
      st[k] = r ? 2 : 0;
      if (r) tsize[k] = 0;
   }
   while (st[0] == 0 || st[1] == 0) {
      bool run[2];
      for (int k = 0; k < 2; k++) run[k] = st[k] == 0 && R[k]->iter < R[k]->maxits;
      for (int k = 0; k < 2; k++)
         if (st[k] == 0 && !run[k]) st[k] = 1;
      if (!run[0] && !run[1]) break;
      for (int k = 0; k < 2; k++)
         if (run[k]) R[k]->step_begin();
      if (run[0] && run[1]) {
         const double* xs[2] = {R[0]->wv, R[1]->wv};
         double* ys[2] = {R[0]->z, R[1]->z};
         if (additive_matvec_multi(cb.mat, 2, 1.0, xs, 0.0, ys)) return -1;
      } else {
         LanczosRun* Q = run[0] ? R[0] : R[1];
         if (cb.apply(1.0, Q->wv, 0.0, Q->z)) return -1;
      }
      if (run[0] && run[1] && R[0]->fast_ok(true) && R[1]->fast_ok(true)) {
         // both runs' scalars behind one read (each in its half of the scalar buffer)
         constexpr int kR = LanczosRun::kRegion;
         if (R[0]->step_enqueue(true, R[0]->c.scal()) || R[1]->step_enqueue(true, R[1]->c.scal(kR))) return -1;
         std::vector<double> hh(kR + R[1]->region_len(true));
         if (R[0]->c.read(R[0]->c.scal(), (int)hh.size(), hh.data())) return -1;
         for (int k = 0; k < 2; k++) {
            const int r = R[k]->step_after(true, hh.data() + k * kR);
            if (r < 0) return -1;
            if (r) st[k] = 1;
         }
      } else {
         for (int k = 0; k < 2; k++) {
            if (!run[k]) continue;
            const int r = R[k]->step_end(true);
            if (r < 0) return -1;
            if (r) st[k] = 1;
         }
      }
   }
   for (int k = 0; k < 2; k++) {
      if (st[k] == 2) {
         free(relv[k]);
         continue;
      }
      if (R[k]->finish(&prel_res[k], &relv[k], &piter[k], &tsize[k])) return -1;
      free(relv[k]);
   }
   return 0;
}

// ---- stochastic Lanczos quadrature (lanczos.c:421-610) --------------------------------------------
int lanczos_logdet_dev(Callbacks& cb, Callbacks& dcb, func_trace tracefunc, func_logdet logdetfunc,
                       func_dvp dvpfunc, int maxits, int nvecs, const double* radamacher, int print_level,
                       double* logdet, double** dlogdetp)
{
   const size_t n = cb.n;
   const double nall = (double)cb.n_global;  // the 1/n normalisations use the whole problem's n
   Ctx c{current_stream(), n, cb.comm};
   void* prec_data = cb.prec ? cb.pdata : nullptr;
   double* dval = *dlogdetp ? *dlogdetp : (double*)calloc(3, sizeof(double));
   double traces_precond[3] = {0.0, 0.0, 0.0}, logdet_precond = 0.0;
   if (prec_data) {
      double* tp = traces_precond;
      if (tracefunc(prec_data, &tp)) return -1;
      for (int i = 0; i < 3; i++) traces_precond[i] /= nall;
      logdet_precond = logdetfunc(prec_data) / nall;
   }
   const bool dvp_dev = g_cb_mode == 1 || (g_cb_mode == -1 && library_operator((const void*)dvpfunc));
   DevBuf<double> z, x, dAz, px, z2, x2;  // (z2, x2: the second probe of a pair)
   SyncOnExit sync{c.s};
   std::vector<double> hz, hpx;
   if (z.alloc(n) || x.alloc(n) || dAz.alloc(3 * n) || px.alloc(3 * n)) return -1;
   const bool rad_dev = radamacher && is_device_ptr(radamacher);
   double val = 0.0;
   for (int j = 0; j < 3; j++) dval[j] = 0.0;
   // probe i's contribution from its Lanczos run (lanczos.c:525-567); 1: the reference's early return
   auto post = [&](int i, const double* zc, const double* xc, double* TD, double* TE, int tsize) -> int {
      if (dcb.apply(1.0, const_cast<double*>(zc), 0.0, dAz)) return -1;
      while (tsize > 0 && std::isnan(TD[tsize - 1])) tsize--;
      if (tsize == 0) {
         printf("Warning: empty tridiagonal matrix\n");  // lanczos.c:525-529 returns without a result
         return 1;
      }
      std::vector<double> w, TV;
      if (tridiag_eig(tsize, TD, TE, w, TV)) {
         printf("Warning: DSTEV failed at iteration %d/%d\n", i, nvecs);
         return -1;
      }
      // sum_j TV(0, j)^2 log|lambda_j|  (TV column-major, eigenvector j in column j)
      for (int j = 0; j < tsize; j++) val += TV[(size_t)j * tsize] * TV[(size_t)j * tsize] * std::log(std::fabs(w[j]));
      if (prec_data) {
         if (dvp_dev) {
            double* pp = px;
            if (dvpfunc(prec_data, (int)n, nullptr, const_cast<double*>(zc), &pp)) return -1;
         } else {
            hz.resize(n);
            hpx.assign(3 * n, 0.0);
            NFFT4GP_HIP_CHECK(hipMemcpy(hz.data(), zc, sizeof(double) * n, hipMemcpyDeviceToHost));
            double* pp = hpx.data();
            if (dvpfunc(prec_data, (int)n, nullptr, hz.data(), &pp)) return -1;
            NFFT4GP_HIP_CHECK(hipMemcpy(px, hpx.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice));
         }
      }
      for (int j = 0; j < 3; j++) {
         dval[j] += c.dot(dAz + (size_t)j * n, xc);
         if (prec_data) dval[j] -= c.dot(px + (size_t)j * n, zc);
      }
      return 0;
   };
   // two probes share their matvecs (lanczos_pair_dev) on this library's additive operator when the probes
   // are given (no rand() draws between them) and the runs print nothing per step
   const bool pairs = radamacher && print_level <= 0 && cb.mv_dev &&
                      cb.matvec == (func_symmatvec)&Nfft4GPAdditiveNFFTMatSymv;
   if (pairs && nvecs > 1 && (z2.alloc(n) || x2.alloc(n))) return -1;
   for (int i = 0; i < nvecs;) {
      if (pairs && i + 1 < nvecs) {
         double* zz[2] = {z, z2};
         double* xx[2] = {x, x2};
         for (int k = 0; k < 2; k++) {
            NFFT4GP_HIP_CHECK(hipMemcpyAsync(zz[k], radamacher + (size_t)(i + k) * n, sizeof(double) * n,
                                             rad_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.s));
            NFFT4GP_HIP_CHECK(hipMemsetAsync(xx[k], 0, sizeof(double) * n, c.s));
         }
         double rel_res[2];
         int tsize[2] = {0, 0};
         double* TD[2] = {nullptr, nullptr};
         double* TE[2] = {nullptr, nullptr};
         const double* zc[2] = {z, z2};
         const int rc = lanczos_pair_dev(cb, xx, zc, maxits, print_level, rel_res, tsize, TD, TE);
         int pr = rc ? -1 : 0;
         for (int k = 0; k < 2 && pr == 0; k++) pr = post(i + k, zz[k], xx[k], TD[k], TE[k], tsize[k]);
         for (int k = 0; k < 2; k++) {
            free(TD[k]);
            free(TE[k]);
         }
         if (pr) return pr < 0 ? -1 : 0;
         i += 2;
         continue;
      }
      if (radamacher) {
         NFFT4GP_HIP_CHECK(hipMemcpyAsync(z, radamacher + (size_t)i * n, sizeof(double) * n,
                                          rad_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.s));
      } else {
         // every rank draws the whole probe (the same libc sequence); a row shard keeps its rows
         hz.resize(cb.n_global);
         Nfft4GPVecRadamacher(hz.data(), (int)cb.n_global);
         NFFT4GP_HIP_CHECK(hipMemcpy(z, hz.data() + cb.row_begin, sizeof(double) * n, hipMemcpyHostToDevice));
      }
      NFFT4GP_HIP_CHECK(hipMemsetAsync(x, 0, sizeof(double) * n, c.s));
      double rel_res, *rel_res_v = nullptr, *TD = nullptr, *TE = nullptr;
      int niter = 0, tsize = 0;
      if (lanczos_dev(cb, x, z, maxits, maxits, 0, DBL_EPSILON, &rel_res, &rel_res_v, &niter, &tsize, &TD, &TE,
                      print_level))
         return -1;
      free(rel_res_v);
      const int pr = post(i, z, x, TD, TE, tsize);
      free(TD);
      free(TE);
      if (pr) return pr < 0 ? -1 : 0;
      i++;
   }
   double scale = 1.0 / (double)nvecs;
   val *= scale;
   scale /= nall;
   for (int j = 0; j < 3; j++) dval[j] *= scale;
   val += logdet_precond;
   for (int j = 0; j < 3; j++) dval[j] += traces_precond[j];
   *logdet = val;
   if (!*dlogdetp) *dlogdetp = dval;
   return 0;
}

}  // namespace nfft4gp_amd

extern "C" {

int Nfft4GPSolverLanczos(void* mat_data, int n, func_symmatvec matvec, void* prec_data, func_solve precondfunc,
                         double* x, double* rhs, int wsize, int maxits, int atol, double tol, double* prel_res,
                         double** prel_res_v, int* piter, int* tsize, double** TDp, double** TEp, int print_level)
{
   RandScope rand_scope;  // libc rand() as the reference draws it (internal.h)
   if (!need_device("Nfft4GPSolverLanczos")) return -1;
   Callbacks cb;
   if (!make_callbacks(cb, n, matvec, mat_data, precondfunc, prec_data)) return -1;
   Vec vx, vb;
   if (vx.open(x, n, true) || vb.open(rhs, n, true)) return -1;
   int rc = lanczos_dev(cb, vx.d, vb.d, wsize, maxits, atol, tol, prel_res, prel_res_v, piter, tsize, TDp, TEp,
                        print_level);
   if (rc == 0 && dist_final_check(cb)) rc = -1;
   vb.close(false);
   vx.close(rc == 0);
   return rc;
}

int Nfft4GPLanczosQuadratureLogdet(void* mat_data, void* dmat_data, int n, func_symmatvec matvec,
                                   func_symmatvec dmatvec, void* prec_data, func_solve precondfunc,
                                   func_trace tracefunc, func_logdet logdetfunc, func_dvp dvpfunc, int maxits,
                                   int nvecs, double* radamacher, int print_level, double* logdet, double** dlogdetp)
{
   RandScope rand_scope;  // libc rand() as the reference draws it (internal.h)
   if (!need_device("Nfft4GPLanczosQuadratureLogdet")) return -1;
   Callbacks cb, dcb;
   if (!make_callbacks(cb, n, matvec, mat_data, precondfunc, prec_data) ||
       !make_callbacks(dcb, n, dmatvec, dmat_data, nullptr, nullptr))
      return -1;
   dcb.out_mult = 3;
   const int rc = lanczos_logdet_dev(cb, dcb, tracefunc, logdetfunc, dvpfunc, maxits, nvecs, radamacher, print_level,
                                     logdet, dlogdetp);
   return rc == 0 && dist_final_check(cb) ? -1 : rc;
}

}  // extern "C"
