// The small least-squares problem of FGMRES (fgmres.c:160-235), host arithmetic only: the Hessenberg columns come
// in one at a time, each is rotated by the earlier Givens rotations and closed by a new one, and the rotated
// right-hand side gives the residual estimate; at the end of a cycle the triangle is back-substituted.  Every
// FGMRES driver of krylov.hip feeds one of these; tests/test_fgmres_lsq_host.py runs it without a GPU
// (Nfft4GPAmdDebugGivensLsq).  Standard library only.
#pragma once

#include <cfloat>
#include <cmath>
#include <utility>
#include <vector>

namespace nfft4gp_amd {

struct GivensLsq {
   std::vector<double> cs, sn, rs;
   std::vector<std::vector<double>> H;  // H[i - 1]: rotated column i - 1 (i + 1 entries)

   // a cycle begins with the residual norm
   void start(double normr)
   {
      rs.assign(1, normr);
      H.clear();
      cs.clear();
      sn.clear();
   }
   int cols() const { return (int)H.size(); }
   // column i - 1 (i = cols() + 1) from its i + 1 raw entries.  false: breakdown (fgmres.c:179-182), nothing
   // changed; else *normr = the residual estimate |rs[i]|
   bool push(const double* col, double* normr)
   {
      const int i = cols() + 1;
      std::vector<double> Hc(col, col + i + 1);
      for (int j = 1; j < i; j++) {
         const double hii = Hc[j - 1];
         Hc[j - 1] = cs[j - 1] * hii + sn[j - 1] * Hc[j];
         Hc[j] = -sn[j - 1] * hii + cs[j - 1] * Hc[j];
      }
      const double hii = Hc[i - 1], hii1 = Hc[i];
      const double gam = std::sqrt(hii * hii + hii1 * hii1);
      if (std::fabs(gam) < DBL_EPSILON) return false;
      cs.push_back(hii / gam);
      sn.push_back(hii1 / gam);
      rs.push_back(-sn[i - 1] * rs[i - 1]);
      rs[i - 1] = cs[i - 1] * rs[i - 1];
      Hc[i - 1] = cs[i - 1] * hii + sn[i - 1] * hii1;
      H.push_back(std::move(Hc));
      *normr = std::fabs(rs[i]);
      return true;
   }
   // y[0..i) of the first i columns (fgmres.c:221-229)
   std::vector<double> solve(int i) const
   {
      std::vector<double> y(rs.begin(), rs.begin() + i);
      if (i <= 0) return y;
      y[i - 1] /= H[i - 1][i - 1];
      for (int k = i - 2; k >= 0; k--) {
         for (int j = k + 1; j < i; j++) y[k] -= H[j][k] * y[j];
         y[k] /= H[k][k];
      }
      return y;
   }
};

}  // namespace nfft4gp_amd
