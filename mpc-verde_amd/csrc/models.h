// models.h -- stage models of the fused solve kernel.
//
// A model supplies NX, NU, the structural masks of its Jacobians, a per-lane context
// (what node k of instance `inst` needs: references, stage matrices) and two stage
// functions: value (F, q) and derivatives (F, q, A, B, grad q, exact Hessian of
// fs*q + lam^T F).  The solver kernel (solver.hip) is written once against this.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "riccati.h"
#include "solver.h"
#include "unicycle.h"


namespace mpcx {

// ------------------------------------------------------------------------------------
// Unicycle (Casadi/multiple_shooting_casadi.py:68-114; Trajectory_tracking.py:40-61)
// A = I + a02 e0 e2^T + a12 e1 e2^T,  B[2][0] = 0  (structural zeros as masks)
// ------------------------------------------------------------------------------------
struct UnicycleModel {
  static constexpr int NX = 3, NU = 2;
  static constexpr unsigned long long AMASK = (1ull << 0) | (1ull << 2) | (1ull << 4) | (1ull << 5) | (1ull << 8);
  static constexpr unsigned long long BMASK = (1ull << 0) | (1ull << 1) | (1ull << 2) | (1ull << 3) | (1ull << 5);
  static constexpr unsigned long long AONE = (1ull << 0) | (1ull << 4) | (1ull << 8);  // A's unit diagonal
  // the line search's first trial evaluates derivatives, not just values: accepted (the
  // usual case) it is the next iteration's evaluation, which is then skipped
  static constexpr bool kEvalInSearch = true;
  // second-order correction (IPOPT max_soc): not here -- the first trial's evaluation replaces
  // the current point's derivatives, and config-2/3 solves do not reach it
  static constexpr bool kSOC = false;
  // IPOPT's soft restoration and restoration phase (resto.h, the resume launch): a warm-started
  // closed-loop solve that sits at its optimum to rounding level can fail the filter line
  // search on noise in theta (tests/test_gpu_hard.py); IPOPT recovers it there
  static constexpr bool kResto = true;
  // variable bounds in LDS, re-read per phase (kernels.h LdsCol): removes the kernel's scratch
  // spills but measured 1-2 % slower on config 2 (LDS latency on the line search), so off
  static constexpr bool kBoundsLds = false;
  // backward Riccati recursion as a log-depth scan (pscan.h) instead of N dependent steps
  static constexpr bool kParallelRiccati = false;
  // a 32-lane group widened to a whole wave runs as two replicas that split the sequential work
  // (kernels.h R = 2): configs 1-2 (N <= 30) at batches below two waves per SIMD
  static constexpr bool kReplicate = true;
  // the sequential Riccati recursion spread over 16-lane rows (rowchain.h; bit-identical to
  // riccati_step) in the single-wave groups of 32 and 64 lanes
  static constexpr bool kRowChain = true;
  struct Ctx {
    double xr[3], ur[2];
  };
  // Jacobian/Hessian operands of the Newton step live in the kernel's registers
  static constexpr bool kTableJac = false, kTableHess = false;
  static constexpr int kTrigSlots = 0;  // no LDS value cache
  __device__ __forceinline__ static const double* jacA(const Ctx&, const double* A) { return A; }
  __device__ __forceinline__ static const double* jacB(const Ctx&, const double* B) { return B; }
  __device__ __forceinline__ static const double* hessW(const Ctx&, const double* H) { return H; }
  __device__ __forceinline__ static void load_ctx(const ModelArgs& a, int inst, const double* P, int k, bool hasU, Ctx& c) {
    for (int i = 0; i < 3; ++i) c.xr[i] = 0.0;
    c.ur[0] = c.ur[1] = 0.0;
    if (a.p_layout == 0) {
      for (int i = 0; i < 3; ++i) c.xr[i] = P[3 + i];
    } else if (hasU) {
      for (int i = 0; i < 3; ++i) c.xr[i] = P[3 + 5 * k + i];
      for (int i = 0; i < 2; ++i) c.ur[i] = P[3 + 5 * k + 3 + i];
    }
  }
  __device__ __forceinline__ static void derivs(const ModelArgs& a, const Ctx& c, const double* z, const double* ln, double fs,
                                double* xf, double& q, double* A, double* Bm, double* g, double* H) {
    const double u2[2] = {z[3], z[4]};
    uni_derivs_moments<0>(a.sp, z, u2, c.xr, c.ur, ln, fs, xf, q, A, Bm, g, H);  // weighted moments (unicycle.h)
  }
  // the same with the moments summed in the replicated groups' two halves: the 32-lane groups,
  // which a small batch runs replicated (stage_derivs below), so that a node's bits do not depend
  // on the batch it is solved in
  __device__ __forceinline__ static void derivs_halves(const ModelArgs& a, const Ctx& c, const double* z,
                                                       const double* ln, double fs, double* xf, double& q, double* A,
                                                       double* Bm, double* g, double* H) {
    const double u2[2] = {z[3], z[4]};
    uni_derivs_moments<1>(a.sp, z, u2, c.xr, c.ur, ln, fs, xf, q, A, Bm, g, H);
  }
  // the same evaluation split between the two replicas of a replicated lane group (kernels.h R = 2;
  // every lane of the wave must call it)
  __device__ __forceinline__ static void derivs_rep(const ModelArgs& a, const Ctx& c, const double* z, const double* ln,
                                                    double fs, double* xf, double& q, double* A, double* Bm, double* g,
                                                    double* H, int rho) {
    const double u2[2] = {z[3], z[4]};
    uni_derivs_moments<2>(a.sp, z, u2, c.xr, c.ur, ln, fs, xf, q, A, Bm, g, H, rho);
  }
  __device__ __forceinline__ static void value(const ModelArgs& a, const Ctx& c, const double* z, double* xf, double& q) {
    const double u2[2] = {z[3], z[4]};
    uni_value(a.sp, z, u2, c.xr, c.ur, xf, q);
  }
  // Reference tangent of a stage (sens.h sens_p_kernel; no solve kernel calls it): with dc = load_ctx of a
  // direction dp of the parameter row, r = d(grad_z (q + lam^T F))/dp . dp and d = dF/dp . dp (zero: F reads
  // no parameter), at fs = 1.  The node cost in closed form.  The quadrature cost's gradient is exactly
  // affine in (x_ref, u_ref) -- its points s_i(z) do not depend on them -- so r is the difference of derivs'
  // own gradient at the references dc and 0: no second copy of the moment formulas to keep in step with
  // the first, and a zero direction gives exact zeros.
  __device__ __forceinline__ static void ref_tangent(const ModelArgs& a, const Ctx&, const Ctx& dc, const double* z,
                                                     const double* ln, double* r, double* d) {
    for (int i = 0; i < 3; ++i) d[i] = 0.0;
    if (a.sp.cost != 0) {
      for (int i = 0; i < 3; ++i) r[i] = -2.0 * a.sp.Q[i] * dc.xr[i];
      for (int i = 0; i < 2; ++i) r[3 + i] = -2.0 * a.sp.R[i] * dc.ur[i];
      return;
    }
    // (one call site run twice, not two inlined copies: the compiler contracts each copy's products and
    // sums into fmas on its own, and the two gradients of a zero direction would differ by an ulp)
    double g0[5] = {};
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
      Ctx rc;
      for (int i = 0; i < 3; ++i) rc.xr[i] = t == 0 ? 0.0 : dc.xr[i];
      for (int i = 0; i < 2; ++i) rc.ur[i] = t == 0 ? 0.0 : dc.ur[i];
      double xf[3], q, A[9], Bm[6], g[5], H[15];
      derivs(a, rc, z, ln, 1.0, xf, q, A, Bm, g, H);
      for (int i = 0; i < 5; ++i) {
        r[i] = g[i] - g0[i];
        g0[i] = g[i];
      }
    }
  }
  // The transpose of load_ctx (sens.h sens_vjp_kernel): the shared target x_ref, or stage k's own row.
  __device__ __forceinline__ static RefSlot ref_slot(const ModelArgs& a, int k) {
    return a.p_layout == 0 ? RefSlot{3, 3, true} : RefSlot{3 + 5 * k, 5, false};
  }
  // Reference cotangent of a stage (sens.h sens_vjp_kernel; no solve kernel calls it), the transpose of
  // ref_tangent: with r = G dzr, d = D dzr (D = 0) its maps, gzr = G^T z~ + D^T lam~ for NX columns at once
  // (xt: 3 x 3, ut: 2 x 3, gzr: 5 x 3, row = variable, column = cotangent; a column's bits do not depend
  // on the others).  Node cost: -2 wgt_i z~_i.  Quadrature cost: the columns of G are derivs' gradient at
  // the unit references minus the one at 0 (ref_tangent's argument: exactly affine), one call site run
  // six times; a zero cotangent meets only products with 0.
  __device__ __forceinline__ static void ref_cotangent(const ModelArgs& a, const Ctx&, const double* z, const double* ln,
                                                       const double* xt, const double* ut, const double*, double* gzr) {
    if (a.sp.cost != 0) {
      for (int c = 0; c < 3; ++c) {
        for (int i = 0; i < 3; ++i) gzr[i * 3 + c] = -2.0 * a.sp.Q[i] * xt[i * 3 + c];
        for (int i = 0; i < 2; ++i) gzr[(3 + i) * 3 + c] = -2.0 * a.sp.R[i] * ut[i * 3 + c];
      }
      return;
    }
    double g0[5] = {};
    for (int i = 0; i < 15; ++i) gzr[i] = 0.0;
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {  // t = 0: the references 0; t = j + 1: the unit reference j
      Ctx rc;
      for (int i = 0; i < 3; ++i) rc.xr[i] = (t == i + 1) ? 1.0 : 0.0;
      for (int i = 0; i < 2; ++i) rc.ur[i] = (t == i + 4) ? 1.0 : 0.0;
      double xf[3], q, A[9], Bm[6], g[5], H[15];
      derivs(a, rc, z, ln, 1.0, xf, q, A, Bm, g, H);
      double col[5];  // column t - 1 of G (t = 0: g0 is kept)
      for (int i = 0; i < 5; ++i) {
        col[i] = g[i] - g0[i];
        g0[i] = (t == 0) ? g[i] : g0[i];
      }
      for (int c = 0; c < 3; ++c) {
        double e = col[0] * xt[c];
        for (int i = 1; i < 3; ++i) e = fma(col[i], xt[i * 3 + c], e);
        for (int i = 0; i < 2; ++i) e = fma(col[3 + i], ut[i * 3 + c], e);
        for (int j = 0; j < 5; ++j) gzr[j * 3 + c] = (t == j + 1) ? e : gzr[j * 3 + c];
      }
    }
  }
  // The model row of a stage (sens.h sens_mdl_kernel): the unicycle has no constants, so no such launch.
  static constexpr int NTH = 0;
  // The weight row of a stage: (Q_0..Q_2, R_0, R_1).
  static constexpr int NWT = 5;
  // Weight tangent of a stage (sens.h sens_wt_kernel; no solve kernel calls it): r = d(grad_z q)/d(Q, R) . dwt
  // at fs = 1; F reads no weight, so d = 0 and the multipliers do not enter.  The node cost in closed form,
  // 2 dwt_i e_i with e the residuals derivs forms.  The quadrature cost's gradient is exactly linear and
  // homogeneous in (Q, R) -- its points do not depend on them -- so r is derivs' own gradient with the
  // direction in the weights' place and zero multipliers: one call site, no second copy of the moment
  // formulas, and a zero direction meets only products with 0.
  __device__ __forceinline__ static void weight_tangent(const ModelArgs& a, const Ctx& c, const double* z,
                                                        const double* dwt, double* r) {
    if (a.sp.cost != 0) {
      for (int i = 0; i < 3; ++i) r[i] = 2.0 * dwt[i] * (z[i] - c.xr[i]);
      for (int i = 0; i < 2; ++i) r[3 + i] = 2.0 * dwt[3 + i] * (z[3 + i] - c.ur[i]);
      return;
    }
    ModelArgs wa = a;
    for (int i = 0; i < 3; ++i) wa.sp.Q[i] = dwt[i];
    for (int i = 0; i < 2; ++i) wa.sp.R[i] = dwt[3 + i];
    const double l0[3] = {};
    double xf[3], q, A[9], Bm[6], H[15];
    derivs(wa, c, z, l0, 1.0, xf, q, A, Bm, r, H);
  }
  // Weight cotangent of a stage (sens.h sens_wt_vjp_kernel; no solve kernel calls it), the transpose of
  // weight_tangent for NX columns at once (xt: 3 x 3, ut: 2 x 3, gwt: 5 x 3, row = weight, column =
  // cotangent; a column's bits do not depend on the others).  Node cost: 2 z~_i e_i.  Quadrature cost:
  // row i is z~^T (derivs' gradient at the unit weight i), one call site run five times; a zero
  // cotangent meets only products with 0.
  __device__ __forceinline__ static void weight_cotangent(const ModelArgs& a, const Ctx& c, const double* z,
                                                          const double* xt, const double* ut, double* gwt) {
    if (a.sp.cost != 0) {
      for (int cc = 0; cc < 3; ++cc) {
        for (int i = 0; i < 3; ++i) gwt[i * 3 + cc] = 2.0 * xt[i * 3 + cc] * (z[i] - c.xr[i]);
        for (int i = 0; i < 2; ++i) gwt[(3 + i) * 3 + cc] = 2.0 * ut[i * 3 + cc] * (z[3 + i] - c.ur[i]);
      }
      return;
    }
    for (int i = 0; i < 15; ++i) gwt[i] = 0.0;
    const double l0[3] = {};
#pragma unroll 1
    for (int t = 0; t < 5; ++t) {  // the unit weight t
      ModelArgs wa = a;
      for (int i = 0; i < 3; ++i) wa.sp.Q[i] = (t == i) ? 1.0 : 0.0;
      for (int i = 0; i < 2; ++i) wa.sp.R[i] = (t == i + 3) ? 1.0 : 0.0;
      double xf[3], q, A[9], Bm[6], g[5], H[15];
      derivs(wa, c, z, l0, 1.0, xf, q, A, Bm, g, H);
      for (int cc = 0; cc < 3; ++cc) {
        double e = g[0] * xt[cc];
        for (int i = 1; i < 3; ++i) e = fma(g[i], xt[i * 3 + cc], e);
        for (int i = 0; i < 2; ++i) e = fma(g[3 + i], ut[i * 3 + cc], e);
        for (int j = 0; j < 5; ++j) gwt[j * 3 + cc] = (t == j) ? e : gwt[j * 3 + cc];
      }
    }
  }
};

// The same model for problems without state bounds (configs 1 and 2: X free, |v| <= 1,
// |w| <= pi/4): the launch picks it when no node has a finite state bound, and every state-bound
// term folds away at compile time (kernels.h kXB).
struct UnicycleFreeModel : UnicycleModel {
  static constexpr bool kXBounds = false;
};

// The same model with the backward Riccati recursion as a log-depth scan (pscan.h).  The scan's
// cost is ceil(log2(N+1)) combine levels whatever N is, the sequential chain's is N steps, so the
// launch picks this instantiation for longer horizons (solver.hip kUnicycleScanMinN; A/B on one
// MI355X: config 3, N = 30, +6.5 % solves/s; config 2, N = 20, -4 %).
struct UnicycleScanModel : UnicycleModel {
  static constexpr bool kParallelRiccati = true;
  static constexpr bool kReplicate = false;  // no sequential chain to split
  static constexpr bool kRowChain = false;   // the chain is the scan's rare fallback
};

// ------------------------------------------------------------------------------------
// Linear (time-varying) model with quadratic stage cost -- the mpctools LTI/LTV QPs
// (Inverted_pendulum/inverted_pendulum_single_shooting_mpctools.py:19-64,
//  Trajectory Tracking/Trajectory_tracking_dynamic_model.py:117-145):
//   x+ = A_j x + B_j u + c_j,   l = (z - zr_k)^T W_j (z - zr_k),   z = (x, u),
// with j = table index of (instance, stage) and zr_k per-stage references in P.
// ------------------------------------------------------------------------------------
template <int NX_, int NU_>
struct LinearModel {
  static constexpr int NX = NX_, NU = NU_, NZ = NX_ + NU_, NH = NZ * (NZ + 1) / 2;
  static constexpr unsigned long long AMASK = (NX * NX >= 64) ? ~0ull : ((1ull << (NX * NX)) - 1);
  static constexpr unsigned long long BMASK = (1ull << (NX * NU)) - 1;
  static constexpr bool kEvalInSearch = false;  // a value is one mat-vec: nothing to save
  static constexpr bool kSOC = false;           // linear constraints: a full step never increases theta
  struct Ctx {
    const double *A, *B, *c, *W;
    double zr[NZ];
    bool dec;  // my stage's table is decoupled (LinTables::dec_mask)
  };
  // Log-depth Riccati scan (pscan.h), and with it A, B and the stage Hessian 2 W read from the
  // stage tables (global memory, cache-resident) instead of register copies held through the
  // whole iteration, which leaves the registers to the scan (derivs then does not fill A, Bm,
  // H).  Measured (one MI355X): config 4 (NX = 4, N = 50) 9.3 M solves/s sequential, 11.9 M
  // scan with register tables, 12.6 M scan with table operands; config 5 (NX = 5, N = 100)
  // 0.91 M sequential, 0.43 M / 0.87 M with the scan (its 65-double elements still spill), so
  // NX = 5 keeps the sequential recursion and register tables.
  static constexpr bool kScan = NX_ <= 4;
  static constexpr bool kParallelRiccati = kScan, kTableJac = kScan, kTableHess = kScan;
  // Decoupled suffix (solver.hip): the sequential recursion reuses P_k on a suffix of
  // decoupled stages -- the move-blocked stages of the cart-pole QP (lti.py).  Scan models
  // keep their scan.
  static constexpr bool kDecSuffix = !kScan;
  // variable bounds in LDS (kernels.h LdsCol), re-read per phase, instead of 2 NZ doubles of
  // registers held through every phase: A/B on one MI355X, config 5 (LinearModel<5,1>, G = 128)
  // scratch 704 -> 240 B/lane, 116 -> 100 us per IPM iteration (+15 % solves/s); config 4
  // (LinearModel<4,1>, scan) +3.5 %, scratch 404 -> 0 (LinearModel<4,2>: 680 -> 84)
  static constexpr bool kBoundsLds = true;
  static constexpr int kTrigSlots = 0;
  __device__ __forceinline__ static const double* jacA(const Ctx& c, const double* A) { return kTableJac ? c.A : A; }
  __device__ __forceinline__ static const double* jacB(const Ctx& c, const double* B) { return kTableJac ? c.B : B; }
  __device__ __forceinline__ static const double* hessW(const Ctx& c, const double* H) { return kTableHess ? c.W : H; }
  __device__ __forceinline__ static void load_ctx(const ModelArgs& a, int inst, const double* P, int k, bool hasU, Ctx& c) {
    const int N = a.N;
    int j = 0;
    if (hasU) j = min(max(a.lin.tab[(a.lin.per_instance ? (size_t)inst * N : 0) + k], 0), a.lin.n_tab - 1);
    c.A = a.lin.A + (size_t)j * NX * NX;
    c.B = a.lin.B + (size_t)j * NX * NU;
    c.c = a.lin.c + (size_t)j * NX;
    c.W = a.lin.W + (size_t)j * NH;
    c.dec = hasU && j < 64 && ((a.lin.dec_mask >> j) & 1ull);
    for (int i = 0; i < NZ; ++i) c.zr[i] = hasU ? P[NX + NZ * k + i] : 0.0;
  }
  __device__ __forceinline__ static void value(const ModelArgs& a, const Ctx& c, const double* z, double* xf, double& q) {
    double dz[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) dz[i] = z[i] - c.zr[i];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      double acc = c.c[r];
#pragma unroll
      for (int m = 0; m < NX; ++m) acc = fma(c.A[r * NX + m], z[m], acc);
#pragma unroll
      for (int l = 0; l < NU; ++l) acc = fma(c.B[r * NU + l], z[NX + l], acc);
      xf[r] = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      double wi = 0.0;
#pragma unroll
      for (int j = 0; j < NZ; ++j) wi = fma(c.W[symix(i, j, NZ)], dz[j], wi);
      acc = fma(dz[i], wi, acc);
    }
    q = acc;
  }
  __device__ __forceinline__ static void derivs(const ModelArgs& a, const Ctx& c, const double* z, const double* ln, double fs,
                                double* xf, double& q, double* A, double* Bm, double* g, double* H) {
    double dz[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) dz[i] = z[i] - c.zr[i];
    if constexpr (!kTableJac) {
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) A[i] = c.A[i];
#pragma unroll
      for (int i = 0; i < NX * NU; ++i) Bm[i] = c.B[i];
    }
    if constexpr (!kTableHess)
#pragma unroll
      for (int i = 0; i < NH; ++i) H[i] = 2.0 * fs * c.W[i];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      double acc = c.c[r];
#pragma unroll
      for (int m = 0; m < NX; ++m) acc = fma(c.A[r * NX + m], z[m], acc);
#pragma unroll
      for (int l = 0; l < NU; ++l) acc = fma(c.B[r * NU + l], z[NX + l], acc);
      xf[r] = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      double wi = 0.0;
#pragma unroll
      for (int j = 0; j < NZ; ++j) wi = fma(c.W[symix(i, j, NZ)], dz[j], wi);
      g[i] = 2.0 * fs * wi;
      acc = fma(dz[i], wi, acc);
    }
    q = acc;
  }
  // reference tangent (UnicycleModel::ref_tangent): r = -2 W_j dzr_k, d = 0
  __device__ __forceinline__ static void ref_tangent(const ModelArgs&, const Ctx& c, const Ctx& dc, const double*,
                                                     const double*, double* r, double* d) {
#pragma unroll
    for (int i = 0; i < NX; ++i) d[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      double wi = 0.0;
#pragma unroll
      for (int j = 0; j < NZ; ++j) wi = fma(c.W[symix(i, j, NZ)], dc.zr[j], wi);
      r[i] = -2.0 * wi;
    }
  }
  // the transpose of load_ctx: stage k's own references
  __device__ __forceinline__ static RefSlot ref_slot(const ModelArgs&, int k) {
    return RefSlot{NX + NZ * k, NZ, false};
  }
  // reference cotangent (UnicycleModel::ref_cotangent): gzr = -2 W_j z~ (W symmetric), NX columns
  __device__ __forceinline__ static void ref_cotangent(const ModelArgs&, const Ctx& c, const double*, const double*,
                                                       const double* xt, const double* ut, const double*, double* gzr) {
#pragma unroll
    for (int i = 0; i < NZ; ++i)
#pragma unroll
      for (int col = 0; col < NX; ++col) {
        double wi = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) wi = fma(c.W[symix(i, j, NZ)], xt[j * NX + col], wi);
#pragma unroll
        for (int j = 0; j < NU; ++j) wi = fma(c.W[symix(i, NX + j, NZ)], ut[j * NX + col], wi);
        gzr[i * NX + col] = -2.0 * wi;
      }
  }
  // The weight row of a stage: its table W_j, the packed upper triangle (mpcx_set_linear_model's layout).
  static constexpr int NWT = NH;
  // weight tangent (UnicycleModel::weight_tangent): r = 2 dW (z - zr_k), dW symmetric, the sum as derivs forms it
  __device__ __forceinline__ static void weight_tangent(const ModelArgs&, const Ctx& c, const double* z,
                                                        const double* dwt, double* r) {
    double dz[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) dz[i] = z[i] - c.zr[i];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      double wi = 0.0;
#pragma unroll
      for (int j = 0; j < NZ; ++j) wi = fma(dwt[symix(i, j, NZ)], dz[j], wi);
      r[i] = 2.0 * wi;
    }
  }
  // weight cotangent (UnicycleModel::weight_cotangent): gW[a][a] = 2 z~_a e_a, gW[a][b] = 2 (z~_a e_b +
  // z~_b e_a) for a < b (the packed entry stands for both W_ab and W_ba), NX columns (gwt: NH x NX)
  __device__ __forceinline__ static void weight_cotangent(const ModelArgs&, const Ctx& c, const double* z,
                                                          const double* xt, const double* ut, double* gwt) {
    double dz[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) dz[i] = z[i] - c.zr[i];
#pragma unroll
    for (int col = 0; col < NX; ++col) {
      double zt[NZ];
#pragma unroll
      for (int i = 0; i < NZ; ++i) zt[i] = i < NX ? xt[i * NX + col] : ut[(i - NX) * NX + col];
#pragma unroll
      for (int i = 0; i < NZ; ++i)
#pragma unroll
        for (int j = i; j < NZ; ++j)
          gwt[symix(i, j, NZ) * NX + col] = (i == j) ? 2.0 * zt[i] * dz[i] : 2.0 * fma(zt[i], dz[j], zt[j] * dz[i]);
    }
  }
  // The model row of a stage: its tables (A row-major NX NX, B row-major NX NU, c NX), in that order.
  static constexpr int NTH = NX * NX + NX * NU + NX;
  // model tangent (OdeModel::model_tangent) in closed form: d = dA x + dB u + dc at the stage's evaluation
  // point (stage 0: x0), r = (dA^T ln; dB^T ln); the cost reads none of them
  __device__ __forceinline__ static void model_tangent(const ModelArgs&, const Ctx&, const double* z, const double* ln,
                                                       const double* dth, double* r, double* d) {
    const double *dA = dth, *dB = dth + NX * NX, *dc = dth + NX * NX + NX * NU;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double e = dc[i];
#pragma unroll
      for (int m = 0; m < NX; ++m) e = fma(dA[i * NX + m], z[m], e);
#pragma unroll
      for (int l = 0; l < NU; ++l) e = fma(dB[i * NU + l], z[NX + l], e);
      d[i] = e;
    }
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      double e = 0.0;
#pragma unroll
      for (int m = 0; m < NX; ++m) e = fma(i < NX ? dA[m * NX + i] : dB[m * NU + (i - NX)], ln[m], e);
      r[i] = e;
    }
  }
  // model cotangent (OdeModel::model_cotangent): gA[r][m] = lam~_r z_m + ln_r z~_m, gB likewise on the
  // inputs, gc = lam~, NX columns (gth: NTH x NX)
  __device__ __forceinline__ static void model_cotangent(const ModelArgs&, const Ctx&, const double* z, const double* ln,
                                                         const double* xt, const double* ut, const double* lt,
                                                         double* gth) {
#pragma unroll
    for (int col = 0; col < NX; ++col)
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        const double l = lt[r * NX + col];
#pragma unroll
        for (int m = 0; m < NX; ++m) gth[(r * NX + m) * NX + col] = fma(l, z[m], ln[r] * xt[m * NX + col]);
#pragma unroll
        for (int m = 0; m < NU; ++m)
          gth[(NX * NX + r * NU + m) * NX + col] = fma(l, z[NX + m], ln[r] * ut[m * NX + col]);
        gth[(NX * NX + NX * NU + r) * NX + col] = l;
      }
  }
};

// Model::kReplicate if the model declares it: a 32-lane group may run replicated (kernels.h R = 2)
template <class M, class = void>
struct ReplicateOf {
  static constexpr bool value = false;
};
template <class M>
struct ReplicateOf<M, std::void_t<decltype(M::kReplicate)>> {
  static constexpr bool value = M::kReplicate;
};

// The stage evaluation of a group of G lanes, one per node (R = 1).  Where the same group may
// also run replicated -- a replicating model's 32-lane groups, widened to a wave when the batch
// leaves SIMDs idle (solve_group_size) -- the moments are summed in the replicas' two halves, so an
// instance gets the same bits whatever batch (and hence group variant) it is solved in.  Every
// 32-lane launch of such a model is a 16 <= N < 32 group: kernels.h solve_shape never widens a
// 16-lane group (N < 16, summed in one pass at 16 and 64 lanes) to 32.
template <class Model, int G, class... Args>
__device__ __forceinline__ void stage_derivs(Args&&... args) {
  if constexpr (ReplicateOf<Model>::value && G == 32)
    Model::derivs_halves(args...);
  else
    Model::derivs(args...);
}

}  // namespace mpcx
