// fgmres.hip -- restarted flexible GMRES on device vectors: one system with modified Gram-Schmidt, block CGS2 or
// delayed CGS2, and a batch of systems in lockstep.
//
//   Nfft4GPSolverFgmres   SRC/solvers/fgmres.c:3-252   restarted flexible GMRES, MGS without re-orthogonalisation
//                                                      (Nfft4GPModifiedGS, SRC/linearalg/matops.c:274-346), the
//                                                      reference's restart and breakdown behaviour
//
// The Givens rotations run on the host (fgmres_lsq.hpp) on scalars read back once per iteration; every vector
// operation is a member of Ctx or BatchCtx (krylov.hpp: the kernels and their launches are krylov.hip's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fgmres_lsq.hpp"
#include "krylov.hpp"

using namespace nfft4gp_amd;

namespace nfft4gp_amd {

// FGMRES orthogonalisation: 0 = the reference's modified Gram-Schmidt (Nfft4GPModifiedGS, one launch per
// basis vector), 1 = block classical Gram-Schmidt passes (the Lanczos re-orthogonalisation's kernels: two
// launches per pass whatever its length), a second pass when the DGKS test asks for it -- Nfft4GPAmdSetFgmresOrtho
int g_fgmres_ortho = -1;
long long g_fgmres_second_passes = 0;  // DGKS re-orthogonalisations taken (ortho 1), Nfft4GPAmdFgmresStats
int fgmres_ortho()
{
   if (g_fgmres_ortho < 0) {
      const char* e = getenv("NFFT4GP_AMD_FGMRES_ORTHO");
      g_fgmres_ortho = (e && (atoi(e) == 1 || atoi(e) == 2)) ? atoi(e) : 0;
   }
   return g_fgmres_ortho;
}

// ---- FGMRES on one system: what every orthogonalisation shares -------------------------------------------------
// One solve's basis V, preconditioned directions Z, residual history and least-squares problem, with the parts of
// fgmres.c:3-252 that do not depend on how a Hessenberg column is obtained.  Every way out of the solve releases
// all of it; the history goes to the caller with the results (done) and never otherwise.
struct FgmresRun {
   Callbacks& cb;
   Ctx& c;
   int print_level;
   double* prel_res;
   double** prel_res_v;
   int* piter;
   DevBuf<double> V, Z;  // without a preconditioner z_i = v_i: the combination reads V and no Z is kept
   double* rel = nullptr;
   double normb = 0.0, normr = 0.0, tolr = 0.0;
   GivensLsq lsq;
   std::vector<double> y;  // the coefficients of x += Z y: kept until the stream is synchronised (Ctx::combine copies)
   Report rep;
   ~FgmresRun()
   {
      (void)hipStreamSynchronize(c.s);
      free(rel);
   }
   int done(double rel_res, int iter)
   {
      *prel_res = rel_res;
      *piter = iter;
      *prel_res_v = rel ? rel : rel_hist(1);  // (the early exits have no history yet)
      rel = nullptr;
      return 0;
   }
   // up to the first cycle: ||b||, the basis (kdim at most kmax, the orthogonalisation's limit), r0 = b - A x in
   // its column 0, the tolerance, the banner.  1: solved already (done was called), -1: error, 0: iterate
   int begin(double* x, const double* rhs, int kdim, int kmax, int maxits, int atol, double tol)
   {
      const size_t n = c.n;
      const double EPS = DBL_EPSILON;
      if (cb.n_global == 0) {  // (a row shard may hold no rows: it still takes part in every all-reduce)
         done(0.0, 0);
         return 1;
      }
      normb = c.norm(rhs);
      if (normb < EPS) {
         NFFT4GP_HIP_CHECK(hipMemsetAsync(x, 0, sizeof(double) * n, c.s));
         done(0.0, 0);
         return 1;
      }
      if (kdim > kmax) {
         fprintf(stderr, "nfft4gp_amd: Nfft4GPSolverFgmres: restart dimension %d above %d\n", kdim, kmax);
         return -1;
      }
      if (V.alloc(n * (size_t)(kdim + 1)) || (cb.prec && Z.alloc(n * (size_t)(kdim + 1)))) return -1;
      c.copy(V, rhs);
      if (cb.apply(-1.0, x, 1.0, V)) return -1;
      normr = c.norm(V);
      if (normr < EPS) {
         done(0.0, 0);
         return 1;
      }
      tolr = atol ? tol : tol * normb;
      rel = rel_hist(maxits + 1);
      rel[0] = normr / normb;
      if (print_level > 0) rep.header("FlexGMRES", kdim, tolr, maxits, normr, rel[0]);
      return 0;
   }
   // the next Hessenberg column of the cycle, at iteration iter (fgmres.c:160-200): the residual estimate, the
   // history and the step's line; false: breakdown
   bool push(const double* col, int iter)
   {
      if (!lsq.push(col, &normr)) return false;
      rel[iter] = normr / normb;
      if (print_level > 0) rep.step(iter, normr, rel[iter], rel[iter - 1]);
      return true;
   }
   void cycle_end(int kdim, int iter)
   {
      if (print_level == 0) rep.cycle_end(kdim, iter, rel[iter]);
   }
   // restart (fgmres.c:236-243): column 0 = rhs - A x through w
   int restart(double* x, const double* rhs, double* w)
   {
      c.copy(V, rhs);
      if (cb.apply(1.0, x, 0.0, w)) return -1;
      return c.sub(V, V, w);
   }
};

// ---- FGMRES with DCGS2 (ortho 2) ------------------------------------------------------------------------------
// The reference's FGMRES (fgmres.c:3-252: the same Givens recurrence, breakdown exit, restart and reporting)
// with the Arnoldi basis orthogonalised by delayed CGS2 (Swirydowicz, Langou, Ananthan, Yang, Thomas 2020):
// step j multiplies the provisional column v_j^0 = u_j / beta_j (once orthogonalised), then ONE sweep forms
// s = V^T v_j^0 (v_j's second pass, delayed) and t = V^T w (w = A v_j^0), and ONE update sweep finalises
// v_j = (v_j^0 - V s) / alpha, alpha^2 = (v_j^0, v_j^0) - |s|^2, and forms the next provisional column
// u = A v_j - V c through the Arnoldi relation A v_j = (w - V H s) / alpha, which gives
// u = (w - V_{<j} t) / alpha - ((v_j^0, w) - s.t) / alpha^2 v_j.  Column j - 1 of H becomes final at step j:
// H(<j, j-1) += beta_j s, H(j, j-1) = beta_j alpha, so the Givens rotation and the residual of iteration j are
// applied one step late (one extra operator application per cycle).  Mathematically CGS2 with a second pass at
// every step; the basis is read twice per step instead of up to four times.
// With a (flexible, right) preconditioner M (fgmres.c:140-146: z = M^-1 v, w = A z) the provisional column's
// z_j^0 = M^-1 v_j^0 is kept, w = A z_j^0, and the finalised direction z_j = (z_j^0 - sum_{k<j} s_k z_k) / alpha
// satisfies A z_j = (w - V H s) / alpha: the same Arnoldi relation, so V, H and the sweeps are unchanged.  z_j is
// never formed: x += Z y is applied as Z^0 c, c from y by the triangular recurrence of the s and alpha (combine).
// The cycles of a solve that FgmresRun::begin has started.
static int fgmres_dcgs2_cycles(FgmresRun& run, double* x, const double* rhs, int kdim, int maxits)
{
   Callbacks& cb = run.cb;
   Ctx& c = run.c;
   const size_t n = c.n;
   double *V = run.V, *Z = run.Z;  // Z: the provisional directions z_j^0 = M^-1 v_j^0 (preconditioned only)
   double& normr = run.normr;
   // Hr: the unrotated Hessenberg (the Arnoldi relation); run.lsq takes each column when it is final
   std::vector<double> Hr((size_t)kdim * (kdim + 1), 0.0);
   // the delayed second pass of each column (s_j, alpha_j): the recurrence from y to Z^0's coefficients
   std::vector<std::vector<double>> spass(kdim + 1);
   std::vector<double> alph(kdim + 1, 1.0);
   std::vector<double>& ccoef = run.y;
   int iter = 0, i = 0;
   double* dsc = c.scal();  // device scalars of step j (m = j + 1): [0, 2m) the sweep, [2m] ||u_j||^2
   std::vector<double> hh, coef;
   bool broke = false, converged = false;
   while (iter < maxits) {
      run.lsq.start(normr);
      c.scale(V, nullptr, 1.0 / normr);
      i = 0;                 // final columns of H in this cycle
      double beta = 0.0;     // ||u_j|| of the provisional column j (j >= 1)
      for (int j = 0;; j++) {
         // step j: column j of V is provisional (j >= 1); column j - 1 of H is completed here
         const bool more = j < kdim && iter + (j > 0 ? 1 : 0) < maxits;  // will column j get a first pass?
         double* vj = V + (size_t)j * n;
         double* w = V + (size_t)(j + 1) * n;
         if (more) {
            if (cb.prec) {
               double* zj = Z + (size_t)j * n;  // z_j^0 = M^-1 v_j^0, w = A z_j^0
               if (cb.solve(zj, vj) || cb.apply(1.0, zj, 0.0, w)) return -1;
            } else if (cb.apply(1.0, vj, 0.0, w)) {
               return -1;
            }
         }
         const int m = j + 1;
         hh.assign(2 * m + 1, 0.0);
         if (c.dots_ab(vj, more ? w : nullptr, V, m, dsc)) return -1;
         if (c.read(dsc, 2 * m + 1, hh.data())) return -1;  // (T is stale when !more)
         if (j > 0) beta = std::sqrt(hh[2 * m]);
         // the delayed second pass of column j: s = hh[0, j), omega = hh[j]
         double alpha = 1.0, ss = 0.0;
         if (j > 0) {
            for (int k = 0; k < j; k++) ss += hh[k] * hh[k];
            const double a2 = hh[j] - ss;
            alpha = a2 > 0.0 ? std::sqrt(a2) : std::sqrt(hh[j]);
            spass[j].assign(hh.begin(), hh.begin() + j);
            alph[j] = alpha;
            // column j - 1 of H is final: H(<j, j-1) += beta s, H(j, j-1) = beta alpha
            double* Hrc = Hr.data() + (size_t)(j - 1) * (kdim + 1);
            for (int k = 0; k < j; k++) Hrc[k] += beta * hh[k];
            Hrc[j] = beta * alpha;
            // fgmres.c:160-200 on that column: the previous rotations, a new one, the residual estimate
            i = j;
            iter++;
            if (!run.push(Hrc, iter)) {
               broke = true;
               break;
            }
            if (normr <= run.tolr) {
               converged = true;
               break;
            }
         }
         if (!more) break;
         // first pass of A v_j: H(<j, j) = (t - (H s))/alpha, H(j, j) = ((v_j^0, w) - s.t)/alpha - (H s)_j)/alpha
         const double* t = hh.data() + m;
         double st = 0.0;
         for (int k = 0; k < j; k++) st += hh[k] * t[k];
         const double vjw = (t[j] - st) / alpha;
         std::vector<double> Hs(m, 0.0);
         for (int q = 0; q < j; q++) {
            const double* Hrq = Hr.data() + (size_t)q * (kdim + 1);
            for (int k = 0; k <= q + 1 && k < m; k++) Hs[k] += Hrq[k] * hh[q];
         }
         double* Hrj = Hr.data() + (size_t)j * (kdim + 1);
         for (int k = 0; k < j; k++) Hrj[k] = (t[k] - Hs[k]) / alpha;
         Hrj[j] = (vjw - Hs[j]) / alpha;
         // update: v_j final, u = w / alpha - sum_{k<j} (t_k / alpha) v_k - (vjw / alpha) v_j
         coef.assign(2 * j + 2, 0.0);
         for (int k = 0; k < j; k++) {
            coef[k] = j > 0 ? hh[k] : 0.0;
            coef[j + k] = t[k] / alpha;
         }
         coef[2 * j] = vjw / alpha;
         coef[2 * j + 1] = 1.0 / alpha;
         if (c.dcgs2_update(V, w, j, coef, dsc + 2 * (m + 1))) return -1;  // ||u_{j+1}||^2 where step j + 1 reads it
      }
      if (broke) break;
      run.cycle_end(kdim, iter);
      if (i > 0) {
         ccoef = run.lsq.solve(i);
         if (cb.prec) {
            // x += sum_j y_j z_j with z_j = (z_j^0 - sum_{k<j} s_jk z_k) / alpha_j: from the last column down,
            // c_j = y_j / alpha_j moves -c_j s_jk onto z_k's coefficient
            for (int q = i - 1; q >= 0; q--) {
               ccoef[q] /= alph[q];
               for (int k = 0; k < q && k < (int)spass[q].size(); k++) ccoef[k] -= ccoef[q] * spass[q][k];
            }
         }
         if (c.combine(x, cb.prec ? Z : V, i, ccoef.data())) return -1;
      }
      if (converged || normr <= run.tolr) break;
      // restart.  The reference keeps the Givens estimate as the new cycle's norm, so its first basis vector is
      // not of unit length; MGS tolerates that, but the block orthogonalisations assume an orthonormal basis, so
      // they restart from the true norm (one dot)
      if (run.restart(x, rhs, V + n)) return -1;
      normr = c.norm(V);
   }
   return run.done(normr / run.normb, iter);
}

// ---- FGMRES (fgmres.c:3-252) on device vectors ----------------------------------------------------
int fgmres_dev(Callbacks& cb, double* x, const double* rhs, int kdim, int maxits, int atol, double tol,
               double* prel_res, double** prel_res_v, int* piter, int print_level)
{
   const int ortho = fgmres_ortho();
   Ctx c{current_stream(), cb.n, cb.comm};
   FgmresRun run{cb, c, print_level, prel_res, prel_res_v, piter};
   // the step's device scalars: i + 1 (MGS), 2 i + 4 (block CGS2), 2 (i + 1) + 1 (DCGS2) of Ctx::kScal
   const int kmax = ortho ? Ctx::kScal / 2 - 2 : Ctx::kScal - 2;
   const int rc0 = run.begin(x, rhs, kdim, kmax, maxits, atol, tol);
   if (rc0) return rc0 < 0 ? -1 : 0;
   if (ortho == 2) return fgmres_dcgs2_cycles(run, x, rhs, kdim, maxits);
   const size_t n = c.n;
   double *V = run.V, *Z = run.Z;
   double& normr = run.normr;
   int iter = 0, i = 0;
   double *v = V, *w = V;
   bool broke = false;
   while (iter < maxits) {
      run.lsq.start(normr);
      c.scale(v, nullptr, 1.0 / normr);
      i = 0;
      while (i < kdim && iter < maxits) {
         i++;
         iter++;
         v = V + (size_t)(i - 1) * n;
         w = V + (size_t)i * n;
         if (cb.prec) {
            double* z = Z + (size_t)(i - 1) * n;
            if (cb.solve(z, v) || cb.apply(1.0, z, 0.0, w)) return -1;
         } else {
            if (cb.apply(1.0, v, 0.0, w)) return -1;
         }
         double* hd = c.scal();
         std::vector<double> hcol(i + 1);
         if (ortho == 0) {
            // Nfft4GPModifiedGS (matops.c:274-346) with k = i-1, no re-orthogonalisation: one launch for the
            // sweep where the grid fits (k_mgs_chain), else one per projection
            const int rc = c.mgs_chain(w, V, i, hd);
            if (rc < 0 || (rc > 0 && c.gs_chain(w, V, i, hd))) return -1;
            if (c.read(hd, i + 1, hcol.data())) return -1;
            if (rc == 0 && c.chain_failed()) return -1;
         } else {
            // classical passes h = V^T w, w -= V h; a second one only when the first dropped ||w|| below 0.7071
            // of its value before it (the DGKS test of the reference's MGS2, matops.c:348-440); H(:, i) = the
            // sum of the passes' projections, ||w|| after the last
            std::vector<double> hh(2 * i + 4);
            if (c.block_cgs2(w, V, i, hd) || c.read(hd, 2 * i + 4, hh.data())) return -1;
            for (int j = 0; j < i; j++) hcol[j] = hh[j];
            hcol[i] = hh[i];
            if (hh[2 * i + 3] != 0.0) {
               for (int j = 0; j < i; j++) hcol[j] += hh[i + 2 + j];
               hcol[i] = hh[2 * i + 2];
               g_fgmres_second_passes++;
            }
         }
         const double t = std::sqrt(hcol[i]);
         hcol[i] = t;
         c.scale(w, nullptr, 1.0 / t);
         if (!run.push(hcol.data(), iter)) {
            broke = true;  // fgmres.c:179-182: leave without updating x
            break;
         }
         if (normr <= run.tolr) break;
      }
      if (broke) break;
      run.cycle_end(kdim, iter);
      run.y = run.lsq.solve(i);
      if (c.combine(x, cb.prec ? Z : V, i, run.y.data())) return -1;
      if (normr <= run.tolr) break;
      // restart; normr keeps the Givens estimate
      v = V;
      if (run.restart(x, rhs, w)) return -1;
      if (ortho) normr = c.norm(v);  // block CGS2: restart from the true norm (see fgmres_dcgs2_cycles)
   }
   return run.done(normr / run.normb, iter);
}

// ---- FGMRES on a batch of right-hand sides (the predict's std solves) ---------------------------------------
// fgmres_dev's MGS iteration (fgmres.c:3-252, ortho 0) for m systems A x_s = b_s at once, in lockstep: every
// running system is at the same step, so each projection is ONE launch over all of them (k_gs_batch, grid.y =
// running systems), the step's Hessenberg entries of every system come back in ONE read, and the operator
// applications go out together (two vectors per pass on this library's additive operator,
// additive_matvec_multi).  Per system the Givens recurrence, breakdown exit, restart and tolerance are
// fgmres_dev's, and so is the arithmetic of every vector kernel (the same bodies and grids): with one system
// the results are fgmres_dev's.  A system leaves the batch when it converges or breaks down, the others go on.
// x0 = 0 (the predict's initial guess, nfft_interface.c:1030-1036), so v_0 = b without an operator application.
// The basis grows in groups of columns as the steps need them (nfft_interface.c:1044 asks for a restart
// dimension of n: no n x n basis is reserved).  x_s = X + s ldx, b_s = B + s ldb.  Lines that fgmres_dev
// would print are kept per system and printed in system order at the end.
int fgmres_batch_dev(Callbacks& cb, int m, double* X, size_t ldx, const double* B, size_t ldb, int kdim, int maxits,
                     int atol, double tol, int print_level, BatchOut& res)
{
   const size_t n = cb.n;
   hipStream_t st = current_stream();
   const double EPS = DBL_EPSILON;
   res.iters.assign(m, 0);
   res.rel_res.assign(m, 0.0);
   if (m <= 0) return 0;
   if (cb.comm || cb.n_global != cb.n) return -1;
   const bool multi = cb.mv_dev && cb.matvec == (func_symmatvec)&Nfft4GPAdditiveNFFTMatSymv;
   DevBuf<double> hd;                   // the step's scalars [j][s]
   std::vector<DevBuf<double>> groups;  // basis column groups (V, then Z when preconditioned)
   std::vector<double*> Vc, Zc;         // column j of every system: Vc[j] + s n
   int hcap = 0;                        // columns of hd
   BatchCtx bc(st, n);                  // (declared after every buffer: it drains the stream before they are freed)
   const int kcyc = std::min(kdim, maxits) + 1;  // columns a cycle can combine
   if (bc.init(m, kcyc, std::min(kdim, maxits) + 2)) return -1;
   // columns [0, need) of the basis (and of Z) allocated, in groups of 16 columns
   auto ensure_cols = [&](int need) -> int {
      constexpr int kG = 16;
      while ((int)Vc.size() < need) {
         const int g = std::min(kG, std::max(1, need + kG - 1 - (int)Vc.size()));
         for (int pass = 0; pass < (cb.prec ? 2 : 1); pass++) {
            groups.emplace_back();
            if (groups.back().alloc(n * m * g)) {
               fprintf(stderr, "nfft4gp_amd: FGMRES batch of %d: no memory for %zu basis columns of %zu\n", m,
                       Vc.size() + g, n);
               return -1;
            }
            double* base = groups.back();
            for (int k = 0; k < g; k++) (pass ? Zc : Vc).push_back(base + (size_t)k * n * m);
         }
      }
      return 0;
   };
   auto ensure_h = [&](int cols) -> int {
      if (cols <= hcap) return 0;
      const int nc = std::max(cols, 2 * hcap);
      DevBuf<double> nh;
      if (nh.alloc((size_t)nc * m)) return -1;
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(st));
      std::swap(hd.p, nh.p);  // (nh frees the old columns)
      hcap = nc;
      return 0;
   };
   std::vector<int> act;
   auto read = [&](const double* d, size_t count, std::vector<double>& h) -> int {
      h.resize(count);
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(h.data(), d, sizeof(double) * count, hipMemcpyDeviceToHost, st));
      NFFT4GP_HIP_CHECK(hipStreamSynchronize(st));
      return 0;
   };
   // y_s = A x_s for the running systems
   auto apply = [&](const std::vector<const double*>& xs, const std::vector<double*>& ys) -> int {
      if (multi) return additive_matvec_multi(cb.mat, (int)xs.size(), 1.0, xs.data(), 0.0, ys.data());
      for (size_t k = 0; k < xs.size(); k++)
         if (cb.apply(1.0, const_cast<double*>(xs[k]), 0.0, ys[k])) return -1;
      return 0;
   };
   struct Sys {
      double normb = 0, normr = 0, tolr = 0, rel_prev = 0;
      GivensLsq lsq;
      std::string log;  // its report lines
   };
   std::vector<Sys> S(m);
   for (int s = 0; s < m; s++) NFFT4GP_HIP_CHECK(hipMemsetAsync(X + (size_t)s * ldx, 0, sizeof(double) * n, st));
   if (ensure_cols(2) || ensure_h(2)) return -1;
   act.resize(m);
   for (int s = 0; s < m; s++) act[s] = s;
   if (bc.set_active(act)) return -1;
   // ||b_s|| (c.norm: the dot of b with itself), then v_0 = b - A 0 = b
   std::vector<double> hh;
   if (bc.gs(const_cast<double*>(B), ldb, nullptr, 0, nullptr, B, ldb, hd) || read(hd, m, hh)) return -1;
   for (int s = 0; s < m; s++) {
      S[s].normb = std::sqrt(hh[s]);
      S[s].normr = S[s].normb;  // ||v_0|| = ||b||: the same vector
      NFFT4GP_HIP_CHECK(hipMemcpyAsync(Vc[0] + (size_t)s * n, B + (size_t)s * ldb, sizeof(double) * n,
                                       hipMemcpyDeviceToDevice, st));
   }
   act.clear();
   for (int s = 0; s < m; s++) {
      Sys& y = S[s];
      if (y.normb < EPS) continue;  // x = 0 (set above), rel_res 0, 0 iterations
      y.tolr = atol ? tol : tol * y.normb;
      y.rel_prev = y.normr / y.normb;
      if (print_level > 0) Report{&y.log}.header("FlexGMRES", kdim, y.tolr, maxits, y.normr, y.rel_prev);
      act.push_back(s);
   }
   if (bc.set_active(act)) return -1;
   int iter = 0;
   // the end of a cycle of system s after i steps (fgmres.c:212-235): its line, back substitution, x += Z y
   auto finish_cycle = [&](int s, int i) -> int {
      if (print_level == 0) Report{&S[s].log}.cycle_end(kdim, iter, S[s].rel_prev);
      return bc.combine_cols(X + (size_t)s * ldx, cb.prec ? Zc : Vc, (size_t)s * n, i, S[s].lsq.solve(i).data());
   };
   std::vector<double> fac(m, 0.0);
   while (!act.empty() && iter < maxits) {
      for (int s : act) {
         S[s].lsq.start(S[s].normr);
         fac[s] = 1.0 / S[s].normr;
      }
      if (bc.scale(Vc[0], fac)) return -1;
      int i = 0;
      while (!act.empty() && i < kdim && iter < maxits) {
         i++;
         iter++;
         if (ensure_cols(i + 1) || ensure_h(i + 1)) return -1;
         std::vector<const double*> xs;
         std::vector<double*> ys;
         for (int s : act) {
            double* v = Vc[i - 1] + (size_t)s * n;
            if (cb.prec) {
               double* z = Zc[i - 1] + (size_t)s * n;
               if (cb.solve(z, v)) return -1;
               xs.push_back(z);
            } else {
               xs.push_back(v);
            }
            ys.push_back(Vc[i] + (size_t)s * n);
         }
         if (apply(xs, ys)) return -1;
         // Nfft4GPModifiedGS (matops.c:274-346) with k = i - 1: the whole sweep of every running system in one
         // launch where the grid fits (k_mgs_chain), else one launch per projection for all of them
         const bool chain = bc.sweep_fits(i);
         if (chain) {
            if (bc.sweep(Vc, i, hd)) return -1;
         } else {
            for (int j = 0; j < i; j++)
               if (bc.gs(Vc[i], n, j ? Vc[j - 1] : nullptr, n, j ? hd + (size_t)(j - 1) * m : nullptr, Vc[j], n,
                      hd + (size_t)j * m))
                  return -1;
            if (bc.gs(Vc[i], n, Vc[i - 1], n, hd + (size_t)(i - 1) * m, nullptr, 0, hd + (size_t)i * m)) return -1;
         }
         if (read(hd, (size_t)(i + 1) * m, hh)) return -1;
         if (chain && bc.sweep_failed()) {
            fprintf(stderr, "nfft4gp_amd: FGMRES batch: the one-launch MGS sweep's wait gave up\n");
            return -1;
         }
         std::vector<int> keep, conv;
         for (int s : act) {
            Sys& y = S[s];
            const double t = std::sqrt(hh[(size_t)i * m + s]);
            std::vector<double> Hc(i + 1);
            for (int j = 0; j < i; j++) Hc[j] = hh[(size_t)j * m + s];
            Hc[i] = t;
            fac[s] = 1.0 / t;
            if (!y.lsq.push(Hc.data(), &y.normr)) {  // fgmres.c:179-182: leave without updating x
               res.iters[s] = iter;
               res.rel_res[s] = y.normr / y.normb;
               continue;
            }
            const double rel = y.normr / y.normb;
            if (print_level > 0) Report{&y.log}.step(iter, y.normr, rel, y.rel_prev);
            y.rel_prev = rel;
            (y.normr <= y.tolr ? conv : keep).push_back(s);
         }
         if (bc.scale(Vc[i], fac)) return -1;
         for (int s : conv) {  // converged in this cycle: its end
            if (finish_cycle(s, i)) return -1;
            res.iters[s] = iter;
            res.rel_res[s] = S[s].normr / S[s].normb;
         }
         if (keep.size() != act.size()) {
            act = keep;
            if (!act.empty() && bc.set_active(act)) return -1;
         }
      }
      if (act.empty()) break;
      // the cycle ends for every running system together (restart dimension or maxits reached)
      for (int s : act)
         if (finish_cycle(s, i)) return -1;
      if (iter >= maxits) break;
      // restart (fgmres.c:236-243): v = b - A x; normr keeps the Givens estimate
      std::vector<const double*> xs;
      std::vector<double*> ys;
      for (int s : act) {
         xs.push_back(X + (size_t)s * ldx);
         ys.push_back(Vc[1] + (size_t)s * n);
      }
      if (apply(xs, ys)) return -1;
      for (int s : act)
         if (bc.c.sub(Vc[0] + (size_t)s * n, B + (size_t)s * ldb, Vc[1] + (size_t)s * n)) return -1;
   }
   for (int s : act) {
      res.iters[s] = iter;
      res.rel_res[s] = S[s].normr / S[s].normb;
   }
   bool printed = false;
   for (int s = 0; s < m; s++)
      if (!S[s].log.empty()) {
         fputs(S[s].log.c_str(), stdout);
         printed = true;
      }
   if (printed) fflush(stdout);
   return 0;
}

}  // namespace nfft4gp_amd

// FGMRES's least-squares recurrence (GivensLsq, fgmres_lsq.hpp) on the host, for tests/test_fgmres_lsq_host.py: a
// cycle that starts from beta and takes the k columns of the column-major (k + 1) x k upper Hessenberg H in order.
// res[j]: the residual estimate after column j; y[0..k): the back-substituted solution; *breakdown: the column at
// which breakdown was reported (the cycle stops there: y holds the solution of the columns before it, the rest of
// res and y is 0), or -1.  k0 > 0: the same object first runs a cycle on (k0, beta0, H0), as before a restart.
extern "C" int Nfft4GPAmdDebugGivensLsq(int k, double beta, const double* H, int k0, double beta0, const double* H0,
                                        double* res, double* y, int* breakdown)
{
   if (k < 1 || !H || k0 < 0 || (k0 > 0 && !H0) || !res || !y || !breakdown) return -1;
   GivensLsq lsq;
   double normr = 0.0;
   if (k0 > 0) {
      lsq.start(beta0);
      for (int j = 0; j < k0; j++)
         if (!lsq.push(H0 + (size_t)j * (k0 + 1), &normr)) break;
   }
   lsq.start(beta);
   std::fill(res, res + k, 0.0);
   std::fill(y, y + k, 0.0);
   *breakdown = -1;
   for (int j = 0; j < k && *breakdown < 0; j++) {
      if (lsq.push(H + (size_t)j * (k + 1), &normr))
         res[j] = normr;
      else
         *breakdown = j;
   }
   const std::vector<double> sol = lsq.solve(lsq.cols());
   std::copy(sol.begin(), sol.end(), y);
   return 0;
}

extern "C" {

void Nfft4GPAmdSetFgmresOrtho(int ortho) { g_fgmres_ortho = (ortho == 1 || ortho == 2) ? ortho : 0; }

// the second classical passes FGMRES (ortho 1) has taken since the last call (its DGKS test), then reset
long long Nfft4GPAmdFgmresSecondPasses(void)
{
   const long long v = g_fgmres_second_passes;
   g_fgmres_second_passes = 0;
   return v;
}

int Nfft4GPSolverFgmres(void* mat_data, int n, func_symmatvec matvec, void* prec_data, func_solve precondfunc,
                        double* x, double* rhs, int kdim, int maxits, int atol, double tol, double* prel_res,
                        double** prel_res_v, int* piter, int print_level)
{
   if (!need_device("Nfft4GPSolverFgmres")) return -1;
   Callbacks cb;
   if (!make_callbacks(cb, n, matvec, mat_data, precondfunc, prec_data)) return -1;
   Vec vx, vb;
   if (vx.open(x, n, true) || vb.open(rhs, n, true)) return -1;
   int rc = fgmres_dev(cb, vx.d, vb.d, kdim, maxits, atol, tol, prel_res, prel_res_v, piter, print_level);
   if (rc == 0 && dist_final_check(cb)) rc = -1;
   vb.close(false);
   vx.close(rc == 0);
   return rc;
}

}  // extern "C"
