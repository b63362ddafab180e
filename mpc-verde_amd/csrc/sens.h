// sens.h -- sensitivities of the MPC solution to the initial state x0 (the feedback gain), one
// kernel of its own beside the solve kernel.
//
// At a primal-dual point (w, lam_g, lam_x) of the barrier problem the derivative of w with respect
// to x0 = P[:nx] solves the solve kernel's KKT system -- stage Hessians H_k + Sigma_k, Jacobians
// A_k, B_k -- with a right-hand side that lives in stage 0 only (dX_0 = dx0).  One backward Riccati
// sweep (delta = 0, zero gradients and defects: they do not enter the matrix part) gives the gains
// K_k, and the forward sweep is the prefix product of the closed-loop maps,
//   Phi_0 = I,  Phi_{k+1} = (A_k + B_k K_k) Phi_k,   dX_k/dx0 = Phi_k,   dU_k/dx0 = K_k Phi_k.
// Unlike the Newton step of the solve, stage 0 keeps its feedback: K_0 = -Huu'_0^-1 (Hux_0 +
// B_0^T P_1 A_0) is dU_0/dx0 itself (the solve zeroes it, dX_0 being no free direction there).
//
// Lane model as in the solve kernel: a lane group of G = 16/32/64 lanes per instance, lane k owns
// node k.  Always the narrowest group (no widening, no replicas), so an instance's bits do not depend
// on the batch; single-wave groups only (N <= 63).  The evaluation and the backward sweep are the
// solve kernel's own functions (Model::derivs through stage_derivs, backward_chain / riccati_step,
// riccati_gains); the forward sweep is new: a log-depth prefix of NX x NX matrix products over the
// DPP partners of collectives.h.  One step of iterative refinement follows (sens_refine): the KKT
// residuals of the result in twice the working precision, and the Riccati solve of them with the
// same factors as two affine scans -- it takes out the backward sweep's rounding, which an unstable
// open loop amplifies (the move-blocked cart-pole QP: 1e-13 before, 2e-15 after).
// The second kernel of the file, sens_p_kernel (below), solves the same system for
// directions of the whole parameter row: the references and targets beside x0; the third,
// sens_vjp_kernel, the transpose: the gradient of a loss on w for the whole row.
// sens_bnd_kernel and sens_bnd_vjp_kernel are the same pair for directions of the
// box bounds lbw / ubw, for every model; sens_wt_kernel and sens_wt_vjp_kernel for
// directions of the cost weights, through the models' weight_tangent / weight_cotangent hooks; sens_mdl_kernel
// and sens_mdl_vjp_kernel for directions of the model itself -- the ODE models' constants,
// the linear model's stage tables -- through model_tangent / model_cotangent: the first right-hand side with a
// defect term.
// Included by kernels.h.
#pragma once

namespace mpcx {

// out = a b (NX x NX, row-major)
template <int NX>
__device__ __forceinline__ void sens_matmul(const double* a, const double* b, double* out) {
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = a[r * NX] * b[c];
#pragma unroll
      for (int m = 1; m < NX; ++m) e = fma(a[r * NX + m], b[m * NX + c], e);
      out[r * NX + c] = e;
    }
}

// Inclusive prefix product over the lanes of a group: lane k enters with M_k and leaves with
// M_k M_{k-1} ... M_0.  Kogge-Stone inside each 16-lane row, then the previous rows' totals by row
// broadcasts (scan_partner / scan_takes: the partners of the solve kernel's affine-map scan, here
// on matrices only); log2 G levels, every lane busy, no LDS.
template <int NX, int G>
__device__ __forceinline__ void sens_prefix_product(int k, double* Am) {
  auto level = [&](auto dc) __attribute__((always_inline)) {
    constexpr int d = decltype(dc)::value;
    if constexpr (d < G) {
      double Ao[NX * NX];
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) Ao[i] = scan_partner<d>(Am[i]);
      if (scan_takes<d>(k)) {
        double An[NX * NX];
        sens_matmul<NX>(Am, Ao, An);
#pragma unroll
        for (int i = 0; i < NX * NX; ++i) Am[i] = An[i];
      }
    }
  };
  level(std::integral_constant<int, 1>{});
  level(std::integral_constant<int, 2>{});
  level(std::integral_constant<int, 4>{});
  level(std::integral_constant<int, 8>{});
  level(std::integral_constant<int, 16>{});
  level(std::integral_constant<int, 32>{});
}

// The same scan on affine maps x -> M x + V (V: NX x NX, one column per right-hand side): lane k
// enters with (M_k, V_k) and leaves with the composition of the maps of lanes 0..k, so V is the
// state after them from a zero start.
template <int NX, int G>
__device__ __forceinline__ void sens_prefix_affine(int k, double* Am, double* Vm) {
  auto level = [&](auto dc) __attribute__((always_inline)) {
    constexpr int d = decltype(dc)::value;
    if constexpr (d < G) {
      double Ao[NX * NX], Vo[NX * NX];
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) {
        Ao[i] = scan_partner<d>(Am[i]);
        Vo[i] = scan_partner<d>(Vm[i]);
      }
      if (scan_takes<d>(k)) {
        double An[NX * NX];
#pragma unroll
        for (int r = 0; r < NX; ++r)
#pragma unroll
          for (int c = 0; c < NX; ++c) {  // V = M_mine V_partner + V_mine
            double e = Vm[r * NX + c];
#pragma unroll
            for (int m = 0; m < NX; ++m) e = fma(Am[r * NX + m], Vo[m * NX + c], e);
            An[r * NX + c] = e;
          }
#pragma unroll
        for (int i = 0; i < NX * NX; ++i) Vm[i] = An[i];
        sens_matmul<NX>(Am, Ao, An);
#pragma unroll
        for (int i = 0; i < NX * NX; ++i) Am[i] = An[i];
      }
    }
  };
  level(std::integral_constant<int, 1>{});
  level(std::integral_constant<int, 2>{});
  level(std::integral_constant<int, 4>{});
  level(std::integral_constant<int, 8>{});
  level(std::integral_constant<int, 16>{});
  level(std::integral_constant<int, 32>{});
}

// Sum of products in twice the working precision (TwoSum / TwoProduct by fma; the compensated dot
// product): the refinement's residuals cancel to ~1e-13 of their terms, so a plain fma chain would
// return only its own rounding.
struct SensAcc {
  double hi = 0.0, lo = 0.0;
  __device__ __forceinline__ void add(double v) {
#pragma clang fp contract(off)  // (a product fused into these sums would void the error terms)
    const double t = hi + v;
    const double bb = t - hi;
    lo += (hi - (t - bb)) + (v - bb);
    hi = t;
  }
  __device__ __forceinline__ void mad(double a, double b) {
#pragma clang fp contract(off)
    const double pr = a * b;
    const double e = fma(a, b, -pr);
    add(pr);
    lo += e;
  }
  __device__ __forceinline__ double value() const { return hi + lo; }
};

// One step of iterative refinement of (dX_k, dU_k) = (X, U) on the KKT system the sweeps solved.
// With the costates lam_k = P_k dX_k, the residuals of the three block rows of node k --
//   rq_k = Hxx dX_k + Hxu dU_k + A_k^T lam_{k+1} - lam_k   (node N: Sigma_x dX_N - lam_N),
//   rr_k = Hux dX_k + Huu dU_k + B_k^T lam_{k+1},
//   d_k  = A_k dX_k + B_k dU_k - dX_{k+1}
// -- are summed in twice the working precision (SensAcc), node-parallel.  The correction is the
// Riccati solve of these right-hand sides with the factors already formed, and both of its sweeps
// are affine scans over the closed-loop maps Acl_k = A_k + B_k K_k:
//   backward  p_N = rq_N,  p_k = Acl_k^T (p_{k+1} + P_{k+1} d_k) + rq_k + K_k^T rr_k
//             (run on the lanes in reverse order: node k on the lane of node N - k),
//   kf_k = -Huu'_k^{-1} (rr_k + B_k^T (p_{k+1} + P_{k+1} d_k)),
//   forward   dX_0 += 0,  ddX_{k+1} = Acl_k ddX_k + B_k kf_k + d_k,  ddU_k = K_k ddX_k + kf_k.
// The backward sweep's rounding (relative ~1e-16 times the growth of P_k = Q + A^T P A over an
// unstable open loop) is what the step removes; X_0 = I stays exact (its correction is an exact 0).
//
// kRhs (sens_p_kernel): the same system with right-hand sides -- rq_k += Rq_k, rr_k += Rr_k, d_k += Dd_k
// (each NX columns wide, zero where the node has no stage) -- and the costates lam_k = P_k dX_k + pk_k,
// pk being carried: the sweep's p_k is added to it.  From X = (dx0 on node 0, else 0), U = 0, pk = 0
// one call is the Riccati solve of the right-hand sides, a second one its refinement.
template <class Model, int G, bool kRhs = false>
__device__ __forceinline__ void sens_refine(int k, int N, bool hasX, bool hasU, const double* Hd, const double* Aop,
                                            const double* Bop, const double* P, const Fac<Model::NX, Model::NU>& fac,
                                            const double* Kk, const double* Acl, double* X, double* U,
                                            const double* Rq = nullptr, const double* Rr = nullptr,
                                            const double* Dd = nullptr, double* pkc = nullptr) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NP = NX * (NX + 1) / 2, NN = NX * NX;
  auto H = [&](int i, int j) { return Hd[symix(i, j, NZ)]; };
  double Ad[NN], Bd[NX * NU];
#pragma unroll
  for (int i = 0; i < NN; ++i) Ad[i] = (hasU && (Model::AMASK & (1ull << i))) ? Aop[i] : 0.0;
#pragma unroll
  for (int i = 0; i < NX * NU; ++i) Bd[i] = (hasU && (Model::BMASK & (1ull << i))) ? Bop[i] : 0.0;
  // (lanes beyond node N carry zeros; a neighbour group's values never enter: from_next is read
  // only where hasU)
  double Xs[NN], lamk[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) Xs[i] = hasX ? X[i] : 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = P[symix(i, 0, NX)] * Xs[c];
#pragma unroll
      for (int m = 1; m < NX; ++m) e = fma(P[symix(i, m, NX)], Xs[m * NX + c], e);
      if constexpr (kRhs) e += pkc[i * NX + c];
      lamk[i * NX + c] = hasX ? e : 0.0;
    }
  double rq[NN], rr[NU * NX], d[NN];
  {
    double Xn[NN], Ln[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const double xn = from_next(Xs[i]), ln = from_next(lamk[i]);
      Xn[i] = hasU ? xn : 0.0;
      Ln[i] = hasU ? ln : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) {
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        SensAcc q, e;
#pragma unroll
        for (int m = 0; m < NX; ++m) q.mad(H(i, m), Xs[m * NX + c]);
#pragma unroll
        for (int l = 0; l < NU; ++l) q.mad(H(i, NX + l), U[l * NX + c]);
#pragma unroll
        for (int m = 0; m < NX; ++m)
          if (Model::AMASK & (1ull << (m * NX + i))) q.mad(Ad[m * NX + i], Ln[m * NX + c]);
        q.add(-lamk[i * NX + c]);
        if constexpr (kRhs) q.add(Rq[i * NX + c]);
        rq[i * NX + c] = hasX ? q.value() : 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m)
          if (Model::AMASK & (1ull << (i * NX + m))) e.mad(Ad[i * NX + m], Xs[m * NX + c]);
#pragma unroll
        for (int l = 0; l < NU; ++l)
          if (Model::BMASK & (1ull << (i * NU + l))) e.mad(Bd[i * NU + l], U[l * NX + c]);
        e.add(-Xn[i * NX + c]);
        if constexpr (kRhs) e.add(Dd[i * NX + c]);
        d[i * NX + c] = hasU ? e.value() : 0.0;
      }
#pragma unroll
      for (int l = 0; l < NU; ++l) {
        SensAcc r;
#pragma unroll
        for (int m = 0; m < NX; ++m) r.mad(H(NX + l, m), Xs[m * NX + c]);
#pragma unroll
        for (int n = 0; n < NU; ++n) r.mad(H(NX + l, NX + n), U[n * NX + c]);
#pragma unroll
        for (int m = 0; m < NX; ++m)
          if (Model::BMASK & (1ull << (m * NU + l))) r.mad(Bd[m * NU + l], Ln[m * NX + c]);
        if constexpr (kRhs) r.add(Rr[l * NX + c]);
        rr[l * NX + c] = hasU ? r.value() : 0.0;
      }
    }
  }
  // t_k = P_{k+1} d_k
  double t[NN];
  {
    double Pn[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const double pn = from_next(P[i]);
      Pn[i] = hasU ? pn : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        double e = Pn[symix(i, 0, NX)] * d[c];
#pragma unroll
        for (int m = 1; m < NX; ++m) e = fma(Pn[symix(i, m, NX)], d[m * NX + c], e);
        t[i * NX + c] = e;
      }
  }
  // backward sweep on the reversed lanes (k <-> N - k is its own inverse)
  const int src = ((int)(threadIdx.x & 63) & ~(G - 1)) + (k <= N ? N - k : k);
  double pk[NN];
  {
    double Mb[NN], Vb[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        double e = rq[i * NX + c];
#pragma unroll
        for (int l = 0; l < NU; ++l) e = fma(Kk[l * NX + i], rr[l * NX + c], e);
#pragma unroll
        for (int m = 0; m < NX; ++m) e = fma(Acl[m * NX + i], t[m * NX + c], e);
        Vb[i * NX + c] = hasU ? e : rq[i * NX + c];
        Mb[i * NX + c] = hasU ? Acl[c * NX + i] : 0.0;
      }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      Mb[i] = from_lane(Mb[i], src);
      Vb[i] = from_lane(Vb[i], src);
    }
    sens_prefix_affine<NX, G>(k, Mb, Vb);
#pragma unroll
    for (int i = 0; i < NN; ++i) pk[i] = from_lane(Vb[i], src);
  }
  if constexpr (kRhs)
#pragma unroll
    for (int i = 0; i < NN; ++i) pkc[i] += hasX ? pk[i] : 0.0;
  // feed-forward kf_k and the forward sweep's offsets c_k = B_k kf_k + d_k
  double kf[NU * NX], cf[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double s[NX], hu[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double pn = from_next(pk[i * NX + c]);
      s[i] = (hasU ? pn : 0.0) + t[i * NX + c];
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      double e = rr[l * NX + c];
#pragma unroll
      for (int m = 0; m < NX; ++m) e = fma(Bd[m * NU + l], s[m], e);
      hu[l] = e;
    }
    if constexpr (NU == 1) {
      kf[c] = hasU ? -fac.r0 * hu[0] : 0.0;
    } else {
      const double z1 = fac.r1 * fma(-fac.t, hu[0], hu[1]);
      kf[NX + c] = hasU ? -z1 : 0.0;
      kf[c] = hasU ? -fma(fac.r0, hu[0], -fac.t * z1) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double e = d[i * NX + c];
#pragma unroll
      for (int l = 0; l < NU; ++l) e = fma(Bd[i * NU + l], kf[l * NX + c], e);
      cf[i * NX + c] = e;
    }
  }
  // forward sweep of the correction: lane k enters with stage k - 1's map (lane 0: identity, 0)
  double Mf[NN], Vf[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const double m = from_prev(Acl[i]), v = from_prev(cf[i]);
    Mf[i] = (k == 0) ? ((i / NX == i % NX) ? 1.0 : 0.0) : (hasX ? m : 0.0);
    Vf[i] = (k == 0 || !hasX) ? 0.0 : v;
  }
  sens_prefix_affine<NX, G>(k, Mf, Vf);
#pragma unroll
  for (int i = 0; i < NN; ++i) X[i] += hasX ? Vf[i] : 0.0;
#pragma unroll
  for (int l = 0; l < NU; ++l)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = kf[l * NX + c];
#pragma unroll
      for (int m = 0; m < NX; ++m) e = fma(Kk[l * NX + m], Vf[m * NX + c], e);
      U[l * NX + c] += hasU ? e : 0.0;
    }
}

// W, LG, LX: the point (B x nw, B x ng, B x nw, the solve's outputs); DW: B x nw x NX (row = index
// in w) or null; K0: B x NU x NX or null; FLAG: B or null (0 regular, 1 irregular: a bounded
// variable without positive slack, or a stage failing the inertia test -- NaN outputs).
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_kernel(SolveArgs a, const double* __restrict__ W,
                                                  const double* __restrict__ LG, const double* __restrict__ LX,
                                                  double* __restrict__ DW, double* __restrict__ K0,
                                                  int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N, ng = NX * (N + 1);
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  // LDS value cache of the ODE models' derivative passes (ode.h), as the solve kernel sets it up
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];

  // ---- parameters, model context, the point
  const double* Pin = a.P + (size_t)(valid ? inst : 0) * a.p_stride;
  double x0[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) x0[i] = valid ? Pin[i] : 0.0;
  const ModelArgs ma = [&] {
    ModelArgs m = model_args(a);
    if (Model::kTrigSlots > 0) {
      m.tc = tcache + threadIdx.x;
      m.tc_stride = kSBS;
    }
    return m;
  }();
  typename Model::Ctx ctx;
  Model::load_ctx(ma, valid ? inst : 0, Pin, k, hasU, ctx);

  double z[NZ] = {}, lam[NX] = {}, lx[NZ] = {};  // lx = zU - zL of my variables (X_0 has none)
  double lb[NZ], ub[NZ];
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    lb[i] = -1e20;
    ub[i] = 1e20;
  }
  if (hasX) {
    const double* w = W + (size_t)inst * nw;
    const double* l = LX + (size_t)inst * nw;
    const double* lbr = a.lbw + (size_t)inst * a.bnd_row;
    const double* ubr = a.ubw + (size_t)inst * a.bnd_row;
    for (int i = 0; i < NX; ++i) {
      z[i] = w[ixw<NX, NU>(k, i)];
      lam[i] = LG[(size_t)inst * ng + NX * k + i];
      if (XBoundsOf<Model>::value && k > 0) {
        lx[i] = l[ixw<NX, NU>(k, i)];
        lb[i] = lbr[ixw<NX, NU>(k, i)];
        ub[i] = ubr[ixw<NX, NU>(k, i)];
      }
    }
    if (hasU)
      for (int i = 0; i < NU; ++i) {
        z[NX + i] = w[iuw<NX, NU>(k, i)];
        lx[NX + i] = l[iuw<NX, NU>(k, i)];
        lb[NX + i] = lbr[iuw<NX, NU>(k, i)];
        ub[NX + i] = ubr[iuw<NX, NU>(k, i)];
      }
  }

  // ---- evaluation at fs = 1 with the multipliers as returned (the results section of the solve
  //      kernel writes lam / fs and (zU - zL) / fs: at fs = 1 its inverse is the identity); lane 0
  //      evaluates at (x0, U_0), as the solve kernel's stage_point does
  double ln[NX];
  group_next<G, NX>(lam, ln, xw);
  double ze[NZ];
#pragma unroll
  for (int i = 0; i < NX; ++i) ze[i] = (k == 0) ? x0[i] : z[i];
#pragma unroll
  for (int i = 0; i < NU; ++i) ze[NX + i] = z[NX + i];
  double xf[NX], qv, A[NX * NX], Bm[NX * NU], gq[NZ], Hs[NH];
  stage_derivs<Model, G>(ma, ctx, ze, ln, 1.0, xf, qv, A, Bm, gq, Hs);

  // ---- Sigma; a bounded variable without positive slack makes the instance irregular
  double sig[NZ];
  bool okl = true;
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    const bool own = (i < NX) ? hasX : hasU;
    sig[i] = 0.0;
    if (own && lb[i] > -kInfBound) {
      const double s = z[i] - lb[i];
      okl = okl && s > 0.0;
      sig[i] += fmax(-lx[i], 0.0) / s;
    }
    if (own && ub[i] < kInfBound) {
      const double s = ub[i] - z[i];
      okl = okl && s > 0.0;
      sig[i] += fmax(lx[i], 0.0) / s;
    }
  }

  // ---- stage operands: H + Sigma (table-Hessian models: 2 W of the stage table; none at node N)
  const double* Aop = Model::jacA(ctx, A);
  const double* Bop = Model::jacB(ctx, Bm);
  const double* Hsrc = Model::hessW(ctx, Hs);
  double Hd[NH];
#pragma unroll
  for (int i = 0; i < NH; ++i) Hd[i] = hasU ? (Model::kTableHess ? 2.0 * Hsrc[i] : Hsrc[i]) : 0.0;
#pragma unroll
  for (int i = 0; i < NZ; ++i) Hd[symix(i, i, NZ)] += sig[i];

  // ---- backward sweep, delta = 0, no inertia correction: P_N = Sigma_x, zero gradients and defects
  const double zero[NZ] = {};
  double P[NP], p[NX];
  terminal_value<NX>(k, N, sig, 0.0, zero, P, p);
  Fac<NX, NU> fac = {};
  bool okf = true;
  if constexpr (WsStashOf<Model>::value) {
    // (the solve kernel's chain of these models reads its operands from the workspace stash; here
    // they are in registers, so the chain is written out: the same riccati_step, lane j only)
    for (int j = N - 1; j >= 0; --j) {
      double Pin_[NP], pin_[NX];
#pragma unroll
      for (int i = 0; i < NP; ++i) Pin_[i] = from_next(P[i]);
#pragma unroll
      for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
      if (k == j)
        (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, false, AOneOf<Model>::value>(
            Hd, zero, Aop, Bop, zero, Pin_, pin_, P, p, fac);
    }
    okf = !hasU || fac_ok<NX, NU>(fac);
  } else {
    DecSuffix<Model> ds;  // no reused suffix: every step is the full one
    ds.kb = N + 1;
    ds.jc = N;
#pragma unroll
    for (int i = 0; i < (DecSuffixOf<Model>::value ? NX : 1); ++i) ds.vpc[i] = 0.0;
    backward_chain<Model, G>(k, N, hasU, true, ds, Hd, 0.0, zero, Aop, Bop, zero, nullptr, 0, gid, P, p, fac, okf);
  }
  okl = okl && (!hasU || okf);

  // ---- gains on all lanes; K_0 is kept
  double Kk[NU * NX], kf[NU];
  riccati_gains<NX, NU>(fac, Kk, kf);
  (void)kf;
#pragma unroll
  for (int i = 0; i < NU * NX; ++i) Kk[i] = hasU ? Kk[i] : 0.0;

  // ---- forward sweep: lane k enters the prefix product with the closed-loop map of stage k - 1
  //      (lane 0: the identity, so Phi_0 = I exactly)
  double Acl[NX * NX], Am[NX * NX];
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      double e = (Model::AMASK & (1ull << (r * NX + m))) ? Aop[r * NX + m] : 0.0;
#pragma unroll
      for (int l = 0; l < NU; ++l)
        if (Model::BMASK & (1ull << (r * NU + l))) e = fma(Bop[r * NU + l], Kk[l * NX + m], e);
      Acl[r * NX + m] = e;
    }
#pragma unroll
  for (int i = 0; i < NX * NX; ++i) {
    const double prv = from_prev(Acl[i]);
    Am[i] = (k == 0) ? ((i / NX == i % NX) ? 1.0 : 0.0) : prv;
  }
  sens_prefix_product<NX, G>(k, Am);
  // dU_k/dx0 = K_k Phi_k
  double Du[NU * NX];
#pragma unroll
  for (int l = 0; l < NU; ++l)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = Kk[l * NX] * Am[c];
#pragma unroll
      for (int m = 1; m < NX; ++m) e = fma(Kk[l * NX + m], Am[m * NX + c], e);
      Du[l * NX + c] = e;
    }

  // ---- one step of iterative refinement with residuals in twice the working precision
  sens_refine<Model, G>(k, N, hasX, hasU, Hd, Aop, Bop, P, fac, Kk, Acl, Am, Du);

  // ---- regular: every bounded slack positive, every stage's Huu' positive definite, finite results
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NX * NX; ++i) tot += fabs(Am[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(Du[i]);
  const bool regular = gall<G>(okl && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  if (DW) {
    double* dw = DW + (size_t)(valid ? inst : 0) * nw * NX;
    if (hasX)
      for (int i = 0; i < NX; ++i)
        for (int c = 0; c < NX; ++c) dw[(size_t)ixw<NX, NU>(k, i) * NX + c] = regular ? Am[i * NX + c] : nan;
    if (hasU)
      for (int l = 0; l < NU; ++l)
        for (int c = 0; c < NX; ++c) dw[(size_t)iuw<NX, NU>(k, l) * NX + c] = regular ? Du[l * NX + c] : nan;
  }
  if (valid && k == 0) {
    if (K0)
      for (int i = 0; i < NU * NX; ++i) K0[(size_t)inst * NU * NX + i] = regular ? Du[i] : nan;
    if (FLAG) FLAG[inst] = regular ? 0 : 1;
  }
}

// ---------------------------------------------------------------------------------------------------
// Directional sensitivities to the whole parameter row P = (x0, references): dw = (dw*/dP) dP for up
// to NX directions per launch.  A parameter direction is the KKT matrix of sens_kernel
// with another right-hand side: dX_0 = dp[:nx], and per stage r_k = d(grad_z l_k)/dp . dp,
// d_k = df_k/dp . dp from the model's reference tangent (Model::ref_tangent on load_ctx of the
// direction row, which maps a row of either layout onto its stage).  The solve of right-hand sides is
// the refinement's (sens_refine<.., true>): the factors' two affine scans, once from (dX_0 = dx0,
// everything else zero) for the solution and once more for its refinement, so no dependent chain
// beyond the backward factorisation is added.  Every column is an independent right-hand side of the
// scans (a column's bits do not depend on the others; the unused ones are zeros).

// a model whose stage row enters its dynamics or cost hooks (ode.h kHooks): no reference tangent
template <class M, class = void>
struct RefTangentOf {
  static constexpr bool value = true;
};
template <class M>
struct RefTangentOf<M, std::void_t<decltype(M::kHooks)>> {
  static constexpr bool value = !M::kHooks;
};

// The stage operands and Riccati factors of an instance at its point, formed as sens_kernel forms
// them (the same evaluation, Sigma, backward sweep without inertia correction and gains).
template <class Model>
struct SensSys {
  static constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU;
  typename Model::Ctx ctx;
  double ze[NZ], ln[NX];                     // the stage's evaluation point and next costate
  double A[NX * NX], Bm[NX * NU], Hs[NZ * (NZ + 1) / 2];
  double Hd[NZ * (NZ + 1) / 2], P[NX * (NX + 1) / 2], Kk[NU * NX], Acl[NX * NX];
  Fac<NX, NU> fac;
  bool ok;  // every bounded slack of my variables positive, my stage's Huu' positive definite
};

template <class Model, int G>
__device__ __forceinline__ void sens_factor(const SolveArgs& a, const ModelArgs& ma, const double* __restrict__ W,
                                            const double* __restrict__ LG, const double* __restrict__ LX, long gid,
                                            int k, int inst, bool valid, SensSys<Model>& s) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  const int N = a.N;
  const int nw = NX + NZ * N, ng = NX * (N + 1);
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  const double* Pin = a.P + (size_t)(valid ? inst : 0) * a.p_stride;
  double x0[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) x0[i] = valid ? Pin[i] : 0.0;
  Model::load_ctx(ma, valid ? inst : 0, Pin, k, hasU, s.ctx);

  double z[NZ] = {}, lam[NX] = {}, lx[NZ] = {};  // lx = zU - zL of my variables (X_0 has none)
  double lb[NZ], ub[NZ];
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    lb[i] = -1e20;
    ub[i] = 1e20;
  }
  if (hasX) {
    const double* w = W + (size_t)inst * nw;
    const double* l = LX + (size_t)inst * nw;
    const double* lbr = a.lbw + (size_t)inst * a.bnd_row;
    const double* ubr = a.ubw + (size_t)inst * a.bnd_row;
    for (int i = 0; i < NX; ++i) {
      z[i] = w[ixw<NX, NU>(k, i)];
      lam[i] = LG[(size_t)inst * ng + NX * k + i];
      if (XBoundsOf<Model>::value && k > 0) {
        lx[i] = l[ixw<NX, NU>(k, i)];
        lb[i] = lbr[ixw<NX, NU>(k, i)];
        ub[i] = ubr[ixw<NX, NU>(k, i)];
      }
    }
    if (hasU)
      for (int i = 0; i < NU; ++i) {
        z[NX + i] = w[iuw<NX, NU>(k, i)];
        lx[NX + i] = l[iuw<NX, NU>(k, i)];
        lb[NX + i] = lbr[iuw<NX, NU>(k, i)];
        ub[NX + i] = ubr[iuw<NX, NU>(k, i)];
      }
  }

  // evaluation at fs = 1 with the multipliers as returned; lane 0 evaluates at (x0, U_0)
  group_next<G, NX>(lam, s.ln, xw);
#pragma unroll
  for (int i = 0; i < NX; ++i) s.ze[i] = (k == 0) ? x0[i] : z[i];
#pragma unroll
  for (int i = 0; i < NU; ++i) s.ze[NX + i] = z[NX + i];
  double xf[NX], qv, gq[NZ];
  stage_derivs<Model, G>(ma, s.ctx, s.ze, s.ln, 1.0, xf, qv, s.A, s.Bm, gq, s.Hs);

  // Sigma; a bounded variable without positive slack makes the instance irregular
  double sig[NZ];
  bool okl = true;
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    const bool own = (i < NX) ? hasX : hasU;
    sig[i] = 0.0;
    if (own && lb[i] > -kInfBound) {
      const double sl = z[i] - lb[i];
      okl = okl && sl > 0.0;
      sig[i] += fmax(-lx[i], 0.0) / sl;
    }
    if (own && ub[i] < kInfBound) {
      const double sl = ub[i] - z[i];
      okl = okl && sl > 0.0;
      sig[i] += fmax(lx[i], 0.0) / sl;
    }
  }

  // stage operands: H + Sigma (table-Hessian models: 2 W of the stage table; none at node N)
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);
  const double* Hsrc = Model::hessW(s.ctx, s.Hs);
#pragma unroll
  for (int i = 0; i < NH; ++i) s.Hd[i] = hasU ? (Model::kTableHess ? 2.0 * Hsrc[i] : Hsrc[i]) : 0.0;
#pragma unroll
  for (int i = 0; i < NZ; ++i) s.Hd[symix(i, i, NZ)] += sig[i];

  // backward sweep, delta = 0, no inertia correction: P_N = Sigma_x, zero gradients and defects
  const double zero[NZ] = {};
  double p[NX];
  terminal_value<NX>(k, N, sig, 0.0, zero, s.P, p);
  s.fac = {};
  bool okf = true;
  if constexpr (WsStashOf<Model>::value) {
    for (int j = N - 1; j >= 0; --j) {  // (the chain written out, as in sens_kernel)
      double Pin_[NP], pin_[NX];
#pragma unroll
      for (int i = 0; i < NP; ++i) Pin_[i] = from_next(s.P[i]);
#pragma unroll
      for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
      if (k == j)
        (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, false, AOneOf<Model>::value>(
            s.Hd, zero, Aop, Bop, zero, Pin_, pin_, s.P, p, s.fac);
    }
    okf = !hasU || fac_ok<NX, NU>(s.fac);
  } else {
    DecSuffix<Model> ds;  // no reused suffix: every step is the full one
    ds.kb = N + 1;
    ds.jc = N;
#pragma unroll
    for (int i = 0; i < (DecSuffixOf<Model>::value ? NX : 1); ++i) ds.vpc[i] = 0.0;
    backward_chain<Model, G>(k, N, hasU, true, ds, s.Hd, 0.0, zero, Aop, Bop, zero, nullptr, 0, gid, s.P, p, s.fac, okf);
  }
  s.ok = okl && (!hasU || okf);

  // gains on all lanes (K_0 is kept) and the closed-loop maps Acl_k = A_k + B_k K_k
  double kf[NU];
  riccati_gains<NX, NU>(s.fac, s.Kk, kf);
  (void)kf;
#pragma unroll
  for (int i = 0; i < NU * NX; ++i) s.Kk[i] = hasU ? s.Kk[i] : 0.0;
#pragma unroll
  for (int r = 0; r < NX; ++r)
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      double e = (Model::AMASK & (1ull << (r * NX + m))) ? Aop[r * NX + m] : 0.0;
#pragma unroll
      for (int l = 0; l < NU; ++l)
        if (Model::BMASK & (1ull << (r * NU + l))) e = fma(Bop[r * NU + l], s.Kk[l * NX + m], e);
      s.Acl[r * NX + m] = e;
    }
}

// W, LG, LX: the point, as for sens_kernel; DP: B x m x p_stride directions, each a row of P;
// DW: B x nw x m (row = index in w, column = direction); FLAG: B or null (sens_kernel's).  1 <= m <= NX.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_p_kernel(SolveArgs a, const double* __restrict__ W,
                                                    const double* __restrict__ LG, const double* __restrict__ LX,
                                                    const double* __restrict__ DP, int m, double* __restrict__ DW,
                                                    int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per direction: the stage's reference tangent, dx0 on node 0
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double r[NZ] = {}, d[NX] = {}, dx0[NX] = {};
    if (c < m) {  // (launch-uniform)
      const double* dp = DP + ((size_t)(valid ? inst : 0) * m + c) * a.p_stride;
      typename Model::Ctx dc;
      Model::load_ctx(ma, valid ? inst : 0, dp, k, hasU, dc);
      Model::ref_tangent(ma, s.ctx, dc, s.ze, s.ln, r, d);
#pragma unroll
      for (int i = 0; i < NX; ++i) dx0[i] = dp[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = hasU ? r[i] : 0.0;
      Dd[i * NX + c] = hasU ? d[i] : 0.0;
      X[i * NX + c] = (valid && k == 0) ? dx0[i] : 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = hasU ? r[NX + l] : 0.0;
      U[l * NX + c] = 0.0;
    }
  }

  // ---- the Riccati solve of the right-hand sides, then one step of iterative refinement: the same
  //      round twice (residuals of the full system in twice the working precision, their solve by the
  //      two affine scans); dX_0 = dx0 stays exact (its correction is an exact 0)
#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- regular: as sens_kernel
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  double* dw = DW + (size_t)(valid ? inst : 0) * nw * m;
  if (hasX)
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)ixw<NX, NU>(k, i) * m + c] = regular ? X[i * NX + c] : nan;
  if (hasU)
    for (int l = 0; l < NU; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)iuw<NX, NU>(k, l) * m + c] = regular ? U[l * NX + c] : nan;
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------
// Adjoint sensitivities: gP = (dw*/dP)^T g for up to NX cotangents g per launch, each shaped like w
// (DESIGN.md §3.5.2).  The KKT matrix is symmetric, so the transpose solve is sens_p_kernel's Riccati
// solve of right-hand sides with the cotangent in their place: rq_k = gX_k on every node (node N
// included), rr_k = gU_k, d = 0, from a zero start X~_0 = 0 -- no sign is flipped.  With its result
// (X~, U~, p~) and the costates lam~_k = P_k X~_k + p~_k, for every direction (r_k, d_k, dx0) of sens_p
//   <g, dw> = lam~_0^T dx0 + sum_{k<N} (z~_k^T r_k + lam~_{k+1}^T d_k),     z~_k = (X~_k, U~_k),
// and with r_k = G_k dzr_k, d_k = D_k dzr_k the model's reference tangent as matrices the gradient row is
//   gP[:nx] = lam~_0,     gzr_k = G_k^T z~_k + D_k^T lam~_{k+1}  (Model::ref_cotangent),
// placed in the row by the transpose of load_ctx's row -> stage mapping (Model::ref_slot): stage k's own
// entries, or one shared target on which the stages' terms are summed over the lane group.
// W, LG, LX: the point, as for sens_kernel; GW: B x m x nw cotangents; GP: B x m x p_stride, every entry
// written (those no stage owns as 0); FLAG: B or null (sens_kernel's).  1 <= m <= NX.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_vjp_kernel(SolveArgs a, const double* __restrict__ W,
                                                      const double* __restrict__ LG, const double* __restrict__ LX,
                                                      const double* __restrict__ GW, int m, double* __restrict__ GP,
                                                      int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per cotangent: its rows of my node (node N has its X rows too)
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double gx[NX] = {}, gu[NU] = {};
    if (c < m) {  // (launch-uniform)
      const double* gw = GW + ((size_t)(valid ? inst : 0) * m + c) * nw;
      if (hasX)
        for (int i = 0; i < NX; ++i) gx[i] = gw[ixw<NX, NU>(k, i)];
      if (hasU)
        for (int l = 0; l < NU; ++l) gu[l] = gw[iuw<NX, NU>(k, l)];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = gx[i];
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = gu[l];
      U[l * NX + c] = 0.0;
    }
  }

  // ---- the Riccati solve of the right-hand sides and one step of iterative refinement, as sens_p_kernel
#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- costates lam~_k = P_k X~_k + p~_k (sens_refine's own), lam~_{k+1} from the next lane
  double lamk[NN], Ln[NN];
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = s.P[symix(i, 0, NX)] * X[c];
#pragma unroll
      for (int mm = 1; mm < NX; ++mm) e = fma(s.P[symix(i, mm, NX)], X[mm * NX + c], e);
      e += pk[i * NX + c];
      lamk[i * NX + c] = hasX ? e : 0.0;
    }
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const double ln = from_next(lamk[i]);
    Ln[i] = hasU ? ln : 0.0;
  }

  // ---- regular: as sens_kernel
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]) + fabs(lamk[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- contraction with the reference tangent: gzr_k = G_k^T z~_k + D_k^T lam~_{k+1}, all columns
  double gzr[NZ * NX];
  Model::ref_cotangent(ma, s.ctx, s.ze, s.ln, X, U, Ln, gzr);
#pragma unroll
  for (int i = 0; i < NZ * NX; ++i) gzr[i] = hasU ? gzr[i] : 0.0;
  const RefSlot slot = Model::ref_slot(ma, k);  // (shared: launch-uniform)
  if (slot.shared)  // every lane ends with the same bits (the symmetric reduction of collectives.h)
#pragma unroll
    for (int i = 0; i < NZ * NX; ++i) gzr[i] = gsum<G>(gzr[i], xw);

  const int np = a.p_stride;
  const bool mine = slot.shared ? (valid && k == 0) : hasU;  // who writes the references' entries
  const int tail = slot.shared ? slot.off + slot.n : NX + NZ * N;  // the row's entries past the owned ones
  const bool tails = valid && k == (slot.shared ? 0 : N);
#pragma unroll
  for (int c = 0; c < NX; ++c)
    if (c < m) {
      double* gp = GP + ((size_t)(valid ? inst : 0) * m + c) * np;
      if (valid && k == 0)
        for (int i = 0; i < NX; ++i) gp[i] = regular ? lamk[i * NX + c] : nan;
      if (mine)
#pragma unroll
        for (int i = 0; i < NZ; ++i)
          if (i < slot.n) gp[slot.off + i] = regular ? gzr[i * NX + c] : nan;
      if (tails)
        for (int j = tail; j < np; ++j) gp[j] = regular ? 0.0 : nan;
    }
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------
// Sensitivities to the box bounds.  With the complementarity products
// zL_i (w_i - lb_i) and zU_i (ub_i - w_i) held fixed, a direction (dlb, dub) of the bounds, each shaped
// like w, enters the KKT system of sens_p_kernel through the right-hand side alone:
//   r_i = -(sigL_i dlb_i + sigU_i dub_i),   sigL_i = zL_i / (w_i - lb_i),   sigU_i = zU_i / (ub_i - w_i),
// on every bounded variable, the X rows of node N included (rq_N != 0); d_k = 0, dX_0 = 0.  No model
// hook is involved, so every model has these kernels, the path-frame bicycle too.  zL = max(-lam_x, 0)
// and zU = max(lam_x, 0) are sens_factor's one-sided split of the returned multiplier zU - zL: at most
// one of sigL, sigU is non-zero per variable, and their sum is the Sigma of the factors.  On a
// two-sided box the split is wrong by O(mu) (the far side's multiplier mu / slack is dropped), like
// the rest of §3.5.  The transpose (sens_bnd_vjp_kernel): with z~ the adjoint solve of
// sens_vjp_kernel (rq_k = gX_k, rr_k = gU_k, zero start),
//   g_lb_i = -sigL_i z~_i,   g_ub_i = -sigU_i z~_i,   <g, dw> = <g_lb, dlb> + <g_ub, dub>.

// sigL, sigU of my variables from the loads sens_factor makes (SensSys keeps only their sum); zero
// where there is no finite bound, on X_0 and on the lanes beyond the horizon
template <class Model>
__device__ __forceinline__ void sens_bnd_sigma(const SolveArgs& a, const double* __restrict__ W,
                                               const double* __restrict__ LX, int k, int inst, bool hasX, bool hasU,
                                               double* sL, double* sU) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU;
  const int nw = NX + NZ * a.N;
#pragma unroll
  for (int i = 0; i < NZ; ++i) sL[i] = sU[i] = 0.0;
  if (!hasX) return;
  const double* w = W + (size_t)inst * nw;
  const double* l = LX + (size_t)inst * nw;
  const double* lbr = a.lbw + (size_t)inst * a.bnd_row;
  const double* ubr = a.ubw + (size_t)inst * a.bnd_row;
  auto one = [&](int i, int j) {
    const double z = w[j], lx = l[j], lb = lbr[j], ub = ubr[j];
    if (lb > -kInfBound) sL[i] = fmax(-lx, 0.0) / (z - lb);
    if (ub < kInfBound) sU[i] = fmax(lx, 0.0) / (ub - z);
  };
  if (XBoundsOf<Model>::value && k > 0)
    for (int i = 0; i < NX; ++i) one(i, ixw<NX, NU>(k, i));
  if (hasU)
    for (int i = 0; i < NU; ++i) one(NX + i, iuw<NX, NU>(k, i));
}

// W, LG, LX: the point, as for sens_kernel; DLB, DUB: B x m x nw directions of the lower and upper
// bounds, each shaped like w (entries on X_0 and where the bound is not finite are not read);
// DW: B x nw x m (sens_p_kernel's layout); FLAG: B or null (sens_kernel's).  1 <= m <= NX.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_bnd_kernel(SolveArgs a, const double* __restrict__ W,
                                                      const double* __restrict__ LG, const double* __restrict__ LX,
                                                      const double* __restrict__ DLB, const double* __restrict__ DUB,
                                                      int m, double* __restrict__ DW, int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);
  double sL[NZ], sU[NZ];
  sens_bnd_sigma<Model>(a, W, LX, k, inst, hasX, hasU, sL, sU);

  // ---- right-hand sides, one column per direction: r = -(sigL dlb + sigU dub) on my bounded variables
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double r[NZ] = {};
    if (c < m && hasX) {  // (c < m: launch-uniform)
      const double* dl = DLB + ((size_t)inst * m + c) * nw;
      const double* du = DUB + ((size_t)inst * m + c) * nw;
#pragma unroll
      for (int i = 0; i < NZ; ++i) {  // (sigma is zero on the rows of U of node N)
        const int j = (i < NX) ? ixw<NX, NU>(k, i) : iuw<NX, NU>(k, i - NX);
        double e = 0.0;
        if (sL[i] != 0.0) e = sL[i] * dl[j];
        if (sU[i] != 0.0) e = fma(sU[i], du[j], e);
        r[i] = -e;
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = r[i];
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = r[NX + l];
      U[l * NX + c] = 0.0;
    }
  }

  // ---- the Riccati solve of the right-hand sides and one step of iterative refinement, as sens_p_kernel
#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- regular: as sens_p_kernel
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  double* dw = DW + (size_t)(valid ? inst : 0) * nw * m;
  if (hasX)
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)ixw<NX, NU>(k, i) * m + c] = regular ? X[i * NX + c] : nan;
  if (hasU)
    for (int l = 0; l < NU; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)iuw<NX, NU>(k, l) * m + c] = regular ? U[l * NX + c] : nan;
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// W, LG, LX: the point, as for sens_kernel; GW: B x m x nw cotangents shaped like w; GLB, GUB: B x m x nw
// gradient rows with respect to the lower and upper bounds, every entry written (0 on X_0 and where
// the bound is not finite, NaN throughout for an irregular instance); FLAG: B or null.  1 <= m <= NX.
// The regular test looks at the adjoint solution (X~, U~), which is all the outputs are formed from
// (sens_vjp_kernel's also looks at the costates it contracts with).
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_bnd_vjp_kernel(SolveArgs a, const double* __restrict__ W,
                                                          const double* __restrict__ LG, const double* __restrict__ LX,
                                                          const double* __restrict__ GW, int m,
                                                          double* __restrict__ GLB, double* __restrict__ GUB,
                                                          int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);
  double sL[NZ], sU[NZ];
  sens_bnd_sigma<Model>(a, W, LX, k, inst, hasX, hasU, sL, sU);

  // ---- right-hand sides, one column per cotangent, as sens_vjp_kernel
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double gx[NX] = {}, gu[NU] = {};
    if (c < m) {  // (launch-uniform)
      const double* gw = GW + ((size_t)(valid ? inst : 0) * m + c) * nw;
      if (hasX)
        for (int i = 0; i < NX; ++i) gx[i] = gw[ixw<NX, NU>(k, i)];
      if (hasU)
        for (int l = 0; l < NU; ++l) gu[l] = gw[iuw<NX, NU>(k, l)];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = gx[i];
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = gu[l];
      U[l * NX + c] = 0.0;
    }
  }

#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- g_lb = -sigL z~, g_ub = -sigU z~: every lane writes its own variables' entries of every row
  //      (a variable without a finite bound, and X_0: an exact 0)
#pragma unroll
  for (int c = 0; c < NX; ++c)
    if (c < m && hasX) {
      double* gl = GLB + ((size_t)inst * m + c) * nw;
      double* gu = GUB + ((size_t)inst * m + c) * nw;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int j = ixw<NX, NU>(k, i);
        gl[j] = regular ? -sL[i] * X[i * NX + c] : nan;
        gu[j] = regular ? -sU[i] * X[i * NX + c] : nan;
      }
      if (hasU)
#pragma unroll
        for (int l = 0; l < NU; ++l) {
          const int j = iuw<NX, NU>(k, l);
          gl[j] = regular ? -sL[NX + l] * U[l * NX + c] : nan;
          gu[j] = regular ? -sU[NX + l] * U[l * NX + c] : nan;
        }
    }
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------
// Sensitivities to the cost weights: Q, R of the diagonal costs, the stage tables W
// of the linear model.  Only q_k depends on them, and linearly, so a direction of the weights leaves
// the KKT matrix of sens_p_kernel as it is and enters the right-hand side alone:
//   r_k = d(grad_z q_k)/d(weights) . dwt_k  (Model::weight_tangent),   d_k = 0,  dX_0 = 0,  rq_N = 0.
// The transpose (sens_wt_vjp_kernel): with z~ = (X~, U~) the adjoint solve of sens_vjp_kernel,
//   <g, dw> = sum_{k<N} z~_k^T r_k,   so stage k's own row gets  gwt_k = (dr_k/dwt_k)^T z~_k
// (Model::weight_cotangent), and their sum over the stages is the gradient for a direction applied to
// every stage alike: the handle's Q, R.  A weight row has Model::NWT entries.

// W, LG, LX: the point, as for sens_kernel; DWT: B x m x (per_stage ? N : 1) x NWT directions of the
// weight row, one per stage or one used at every stage (launch-uniform; a row that is the same at every
// stage gives the same bits either way: only the address differs); DW: B x nw x m (sens_p_kernel's
// layout, the X_0 rows exact zeros); FLAG: B or null (sens_kernel's).  1 <= m <= NX.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_wt_kernel(SolveArgs a, const double* __restrict__ W,
                                                     const double* __restrict__ LG, const double* __restrict__ LX,
                                                     const double* __restrict__ DWT, int per_stage, int m,
                                                     double* __restrict__ DW, int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX, NWT = Model::NWT;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per direction: the stage's weight tangent at its evaluation point
  const size_t rows = per_stage ? (size_t)N : 1, row = per_stage ? (size_t)k : 0;
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double r[NZ] = {};
    if (c < m && hasU) {  // (c < m: launch-uniform; the hooks exchange nothing between lanes)
      const double* dr = DWT + (((size_t)inst * m + c) * rows + row) * NWT;
      double dwt[NWT];
#pragma unroll
      for (int i = 0; i < NWT; ++i) dwt[i] = dr[i];
      Model::weight_tangent(ma, s.ctx, s.ze, dwt, r);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = hasU ? r[i] : 0.0;
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = hasU ? r[NX + l] : 0.0;
      U[l * NX + c] = 0.0;
    }
  }

  // ---- the Riccati solve of the right-hand sides and one step of iterative refinement, as sens_p_kernel
#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- regular: as sens_p_kernel
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  double* dw = DW + (size_t)(valid ? inst : 0) * nw * m;
  if (hasX)
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)ixw<NX, NU>(k, i) * m + c] = regular ? X[i * NX + c] : nan;
  if (hasU)
    for (int l = 0; l < NU; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)iuw<NX, NU>(k, l) * m + c] = regular ? U[l * NX + c] : nan;
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// W, LG, LX: the point, as for sens_kernel; GW: B x m x nw cotangents shaped like w; GWK: B x m x N x NWT
// gradient rows with respect to every stage's own weight row, or null; GWS: B x m x NWT, their sum over
// the stages (gsum: the same bits whichever lane writes; lane 0 does), or null; every entry of the ones
// given is written, NaN throughout for an irregular instance; FLAG: B or null.  1 <= m <= NX.  The
// regular test is sens_bnd_vjp_kernel's: the adjoint solution is all the outputs are formed from.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_wt_vjp_kernel(SolveArgs a, const double* __restrict__ W,
                                                         const double* __restrict__ LG, const double* __restrict__ LX,
                                                         const double* __restrict__ GW, int m,
                                                         double* __restrict__ GWK, double* __restrict__ GWS,
                                                         int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX, NWT = Model::NWT;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per cotangent, as sens_vjp_kernel
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double gx[NX] = {}, gu[NU] = {};
    if (c < m) {  // (launch-uniform)
      const double* gw = GW + ((size_t)(valid ? inst : 0) * m + c) * nw;
      if (hasX)
        for (int i = 0; i < NX; ++i) gx[i] = gw[ixw<NX, NU>(k, i)];
      if (hasU)
        for (int l = 0; l < NU; ++l) gu[l] = gw[iuw<NX, NU>(k, l)];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = gx[i];
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = gu[l];
      U[l * NX + c] = 0.0;
    }
  }

#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- contraction with the weight tangent: gwt_k = (dr_k/dwt_k)^T z~_k, all columns; zero beyond the
  //      last stage (node N has no cost)
  double gwt[NWT * NX];
  Model::weight_cotangent(ma, s.ctx, s.ze, X, U, gwt);
#pragma unroll
  for (int i = 0; i < NWT * NX; ++i) gwt[i] = hasU ? gwt[i] : 0.0;
  if (GWK && hasU)  // every stage lane writes its own rows
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < m) {
        double* gk = GWK + (((size_t)inst * m + c) * N + k) * NWT;
#pragma unroll
        for (int i = 0; i < NWT; ++i) gk[i] = regular ? gwt[i * NX + c] : nan;
      }
  if (GWS) {  // (launch-uniform) the stage sum: every lane ends with the same bits, lane 0 writes them
#pragma unroll
    for (int i = 0; i < NWT * NX; ++i) gwt[i] = gsum<G>(gwt[i], xw);
    if (valid && k == 0)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) {
          double* gs = GWS + ((size_t)inst * m + c) * NWT;
#pragma unroll
          for (int i = 0; i < NWT; ++i) gs[i] = regular ? gwt[i * NX + c] : nan;
        }
  }
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------
// Sensitivities to the model: the constants par of the ODE models, the stage tables
// (A, B, c) of the linear model.  A model row th_k of stage k enters F_k(z, th) and, where a cost hook reads
// the constants (the path-frame bicycle), q_k(z, th).  Stationarity and the defect of stage k read
//   grad_z q_k + grad_z (lam_{k+1}^T F_k) - (lam_k; 0) = 0,     F_k - x_{k+1} = 0,
// so along a direction dth_k, with the multipliers held fixed, the right-hand sides of sens_p_kernel's system are
//   r_k = [d(grad_z q_k)/dth + d(grad_z (lam_{k+1}^T F_k))/dth] dth_k,    d_k = (dF_k/dth) dth_k
// (Model::model_tangent), dX_0 = 0, nothing on node N: the first right-hand side with Dd != 0.
// The transpose (sens_mdl_vjp_kernel): the KKT matrix K of the unknowns (z, lam) is symmetric and both solves are
// K y + rhs = 0, so with (z~, lam~) the adjoint solve of sens_vjp_kernel (rq_k = gX_k, rr_k = gU_k, d = 0) and
// lam~_k = P_k X~_k + p~_k its costates -- lam~_{k+1} is the unknown paired with the defect row of stage k --
//   <g, dw> = sum_{k<N} (z~_k^T r_k + lam~_{k+1}^T d_k),
//   gth_k = (dr_k/dth_k)^T z~_k + (dd_k/dth_k)^T lam~_{k+1}      (Model::model_cotangent),
// no sign flipped; their sum over the stages is the gradient for a row shared by all stages (the handle's par).
// A model row has Model::NTH entries.

// W, LG, LX: the point, as for sens_kernel; DTH: B x m x (per_stage ? N : 1) x NTH directions of the model
// row, one per stage or one used at every stage (launch-uniform; the same bits either way for a row that is
// the same at every stage); DW: B x nw x m (sens_p_kernel's layout, the X_0 rows exact zeros); FLAG: B or
// null (sens_kernel's).  1 <= m <= NX.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_mdl_kernel(SolveArgs a, const double* __restrict__ W,
                                                      const double* __restrict__ LG, const double* __restrict__ LX,
                                                      const double* __restrict__ DTH, int per_stage, int m,
                                                      double* __restrict__ DW, int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX, NTH = Model::NTH;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per direction: the stage's model tangent at its evaluation point
  const size_t rows = per_stage ? (size_t)N : 1, row = per_stage ? (size_t)k : 0;
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) Rq[i] = Dd[i] = X[i] = pk[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NU * NX; ++i) Rr[i] = U[i] = 0.0;
#pragma unroll 1
  for (int c = 0; c < m; ++c) {  // (one body for the columns: the ODE models' tangent is NZ hyper-dual passes)
    double r[NZ] = {}, d[NX] = {};
    if (hasU) {  // (the hooks exchange nothing between lanes)
      const double* dr = DTH + (((size_t)inst * m + c) * rows + row) * NTH;
      double dth[NTH];
#pragma unroll
      for (int i = 0; i < NTH; ++i) dth[i] = dr[i];
      Model::model_tangent(ma, s.ctx, s.ze, s.ln, dth, r, d);
    }
#pragma unroll
    for (int cc = 0; cc < NX; ++cc)
      if (cc == c) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          Rq[i * NX + cc] = hasU ? r[i] : 0.0;
          Dd[i * NX + cc] = hasU ? d[i] : 0.0;
        }
#pragma unroll
        for (int l = 0; l < NU; ++l) Rr[l * NX + cc] = hasU ? r[NX + l] : 0.0;
      }
  }

  // ---- the Riccati solve of the right-hand sides and one step of iterative refinement, as sens_p_kernel
#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- regular: as sens_p_kernel
  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  double* dw = DW + (size_t)(valid ? inst : 0) * nw * m;
  if (hasX)
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)ixw<NX, NU>(k, i) * m + c] = regular ? X[i * NX + c] : nan;
  if (hasU)
    for (int l = 0; l < NU; ++l)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) dw[(size_t)iuw<NX, NU>(k, l) * m + c] = regular ? U[l * NX + c] : nan;
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

// W, LG, LX: the point, as for sens_kernel; GW: B x m x nw cotangents shaped like w; GTK: B x m x N x NTH
// gradient rows with respect to every stage's own model row, or null; GTS: B x m x NTH, their sum over the
// stages (gsum: the same bits whichever lane writes; lane 0 does), or null; every entry of the ones given is
// written, NaN throughout for an irregular instance; FLAG: B or null.  1 <= m <= NX.  The regular test is
// sens_vjp_kernel's: the adjoint solution and the costates the outputs are formed from.
template <class Model, int G>
__global__ __launch_bounds__(64) void sens_mdl_vjp_kernel(SolveArgs a, const double* __restrict__ W,
                                                          const double* __restrict__ LG, const double* __restrict__ LX,
                                                          const double* __restrict__ GW, int m,
                                                          double* __restrict__ GTK, double* __restrict__ GTS,
                                                          int32_t* __restrict__ FLAG) {
  static_assert(G == 16 || G == 32 || G == 64, "single-wave groups");
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NN = NX * NX, NTH = Model::NTH;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = (int)(gid & (G - 1));  // node of this lane
  const int inst = (int)(gid / G);
  const bool valid = inst < a.B;
  const int N = a.N;
  const int nw = NX + NZ * N;
  const bool hasX = valid && k <= N;
  const bool hasU = valid && k < N;
  XWave<G> xw{nullptr, 0};
  constexpr int kSBS = 64;
  __shared__ double tcache[Model::kTrigSlots > 0 ? Model::kTrigSlots * kSBS : 1];
  const ModelArgs ma = [&] {
    ModelArgs mm = model_args(a);
    if (Model::kTrigSlots > 0) {
      mm.tc = tcache + threadIdx.x;
      mm.tc_stride = kSBS;
    }
    return mm;
  }();
  SensSys<Model> s;
  sens_factor<Model, G>(a, ma, W, LG, LX, gid, k, inst, valid, s);
  const double* Aop = Model::jacA(s.ctx, s.A);
  const double* Bop = Model::jacB(s.ctx, s.Bm);

  // ---- right-hand sides, one column per cotangent, as sens_vjp_kernel
  double Rq[NN], Rr[NU * NX], Dd[NN], X[NN], U[NU * NX], pk[NN];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double gx[NX] = {}, gu[NU] = {};
    if (c < m) {  // (launch-uniform)
      const double* gw = GW + ((size_t)(valid ? inst : 0) * m + c) * nw;
      if (hasX)
        for (int i = 0; i < NX; ++i) gx[i] = gw[ixw<NX, NU>(k, i)];
      if (hasU)
        for (int l = 0; l < NU; ++l) gu[l] = gw[iuw<NX, NU>(k, l)];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      Rq[i * NX + c] = gx[i];
      Dd[i * NX + c] = 0.0;
      X[i * NX + c] = 0.0;
      pk[i * NX + c] = 0.0;
    }
#pragma unroll
    for (int l = 0; l < NU; ++l) {
      Rr[l * NX + c] = gu[l];
      U[l * NX + c] = 0.0;
    }
  }

#pragma unroll 1
  for (int round = 0; round < 2; ++round)
    sens_refine<Model, G, true>(k, N, hasX, hasU, s.Hd, Aop, Bop, s.P, s.fac, s.Kk, s.Acl, X, U, Rq, Rr, Dd, pk);

  // ---- costates lam~_k = P_k X~_k + p~_k (sens_refine's own), lam~_{k+1} from the next lane
  double lamk[NN], Ln[NN];
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double e = s.P[symix(i, 0, NX)] * X[c];
#pragma unroll
      for (int mm = 1; mm < NX; ++mm) e = fma(s.P[symix(i, mm, NX)], X[mm * NX + c], e);
      e += pk[i * NX + c];
      lamk[i * NX + c] = hasX ? e : 0.0;
    }
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const double ln = from_next(lamk[i]);
    Ln[i] = hasU ? ln : 0.0;
  }

  double tot = 0.0;
  if (hasX)
#pragma unroll
    for (int i = 0; i < NN; ++i) tot += fabs(X[i]) + fabs(lamk[i]);
  if (hasU)
#pragma unroll
    for (int i = 0; i < NU * NX; ++i) tot += fabs(U[i]);
  const bool regular = gall<G>(s.ok && tot < INFINITY, xw);  // (tot: false for NaN and Inf)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- contraction with the model tangent: gth_k = (dr_k/dth_k)^T z~_k + (dd_k/dth_k)^T lam~_{k+1}, all
  //      columns; zero beyond the last stage
  double gth[NTH * NX];
#pragma unroll
  for (int i = 0; i < NTH * NX; ++i) gth[i] = 0.0;
  if (hasU) Model::model_cotangent(ma, s.ctx, s.ze, s.ln, X, U, Ln, gth);
  if (GTK && hasU)  // every stage lane writes its own rows
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < m) {
        double* gk = GTK + (((size_t)inst * m + c) * N + k) * NTH;
#pragma unroll
        for (int i = 0; i < NTH; ++i) gk[i] = regular ? gth[i * NX + c] : nan;
      }
  if (GTS) {  // (launch-uniform) the stage sum: every lane ends with the same bits, lane 0 writes them
#pragma unroll
    for (int i = 0; i < NTH * NX; ++i) gth[i] = gsum<G>(gth[i], xw);
    if (valid && k == 0)
#pragma unroll
      for (int c = 0; c < NX; ++c)
        if (c < m) {
          double* gs = GTS + ((size_t)inst * m + c) * NTH;
#pragma unroll
          for (int i = 0; i < NTH; ++i) gs[i] = regular ? gth[i * NX + c] : nan;
        }
  }
  if (valid && k == 0 && FLAG) FLAG[inst] = regular ? 0 : 1;
}

}  // namespace mpcx
