// backward.h -- the backward Riccati sweeps of the solve kernel (kernels.h "Riccati + inertia
// correction"), one function per strategy: backward_scan (Model::kParallelRiccati), backward_rowchain
// and backward_rowchain6 (kRowChain), backward_chain (G <= 64), backward_chain_waves (G > 64), and
// the decoupled suffix of the linear models (kDecSuffix: dec_suffix_*, suffix_scan).  The kernel
// forms the stage operands (Hd = stage Hessian + Sigma + delta, the barrier gradient gp, the
// Jacobians, the defect), picks the strategy and runs the inertia-correction loop around it; every
// strategy leaves on node lane k the value function (P_k, p_k), the step's factors `fac` and the
// lane's inertia verdict `okl`, by the operations of riccati_step (riccati.h): the same bits.
// Operands are arguments (no captures of the kernel's state), so tests/hip/rowchain_check.hip,
// scan_check.hip and suffix_check.hip call the very functions the kernel runs.  Included by kernels.h
// after its stamp macros and model traits.
#pragma once

namespace mpcx {

// Node N's value function P_N = Sigma_x + delta, p_N = barrier gradient; zeros on every other lane
template <int NX>
__device__ __forceinline__ void terminal_value(int k, int N, const double* sgv, double delta, const double* gp,
                                               double* P, double* p) {
  const double dl = (k == N) ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
#pragma unroll
    for (int j = i; j < NX; ++j) P[symix(i, j, NX)] = (i == j) ? dl * (sgv[i] + delta) : 0.0;
    p[i] = dl * gp[i];
  }
}

// ---- workspace chain stash (solver.h ChainRec): one contiguous record per thread (array of
// structures, after the restoration workspace's slot-major part), so the chain's single active lane
// reads its operands from a few cache lines in 16-byte loads instead of one line per value.
// Thread gid's record (16-byte aligned: hipMalloc base, 64-thread-multiple stride, even record
// size); opaque, so no address is hoisted out of the solve loop
template <class Model>
__device__ __forceinline__ const double* chain_record(double* ws, long ws_stride, long gid) {
  constexpr ChainRec rec(Model::NX, Model::NU);
  static_assert(!WsStashOf<Model>::value || rec.size % 2 == 0, "chain stash record: 16-byte aligned");
  double* r = ws + (long)RestoWs::slots(Model::NX, Model::NU) * ws_stride + gid * rec.size;
  asm volatile("" : "+v"(r));
  return (const double*)__builtin_assume_aligned(r, 16);
}
// a lane's Jacobians back from its record r
template <class Model>
__device__ __forceinline__ void chain_record_jac(const double* r, double* Aw, double* Bw) {
  constexpr int NX = Model::NX, NU = Model::NU;
  constexpr ChainRec rec(NX, NU);
#pragma unroll
  for (int i = 0; i < NX * NX; ++i) Aw[i] = (Model::AMASK & (1ull << i)) ? wsload(r, rec.A + i) : 0.0;
#pragma unroll
  for (int i = 0; i < NX * NU; ++i) Bw[i] = (Model::BMASK & (1ull << i)) ? wsload(r, rec.B + i) : 0.0;
}
// Hd = stage Hessian + Sigma + delta from the record r
template <class Model>
__device__ __forceinline__ void stage_hessian_ws(const double* r, double delta, double* Hj) {
  constexpr int NZ = Model::NX + Model::NU;
  constexpr ChainRec rec(Model::NX, Model::NU);
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int jj = i; jj < NZ; ++jj) {
      const int t = symix(i, jj, NZ);
      Hj[t] = wsload(r, rec.H + t);
      if (jj == i) Hj[t] += wsload(r, rec.S + i) + delta;
    }
}

// ---- log-depth associative scan of conditional value functions (pscan.h), then ONE node-parallel
// Riccati step per lane.  `sbuf`: RElem<NX>::NE fields of one double per thread of the block.
// Returns true (group-uniform) when the instance needs the sequential recursion instead: the scan
// is usable only if every stage's R is positive definite, finite, and consistent with the step.
template <class Model, int G, int R>
__device__ __forceinline__ bool backward_scan(int k, int N, bool hasU, bool hasX, const double* Hd, const double* sgv,
                                              double delta, const double* gp, const double* Aop, const double* Bop,
                                              const double* cdef, double* sbuf, XWave<G>& xw, double* P, double* p,
                                              Fac<Model::NX, Model::NU>& fac, bool& okl) {
  constexpr int NX = Model::NX, NU = Model::NU, NP = NX * (NX + 1) / 2;
  constexpr int kSBS = G > 64 ? G : 64;  // threads per block = field stride
  RElem<NX> e;
  bool eok = true;
  if (hasU) {
    eok = relem_stage<NX, NU, Model::AMASK, Model::BMASK>(Hd, gp, Aop, Bop, cdef, e);
  } else {
    relem_identity<NX>(e);
    if (hasX) {  // node N: terminal (0, 0, 0, Sigma_x + delta, barrier gradient)
#pragma unroll
      for (int i = 0; i < NX * NX; ++i) e.A[i] = 0.0;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
#pragma unroll
        for (int j = i; j < NX; ++j) e.J[symix(i, j, NX)] = (i == j) ? sgv[i] + delta : 0.0;
        e.p[i] = gp[i];
      }
    }
  }
  // Hillis-Steele suffix scan over the whole group through the LDS buffer `sbuf`
  // (partner = thread t + d; block-uniform trip count, two barriers per level)
  const int t = (int)threadIdx.x;
  for (int d = 1; d < G && d <= N; d <<= 1) {
    relem_store<NX>(e, sbuf, kSBS, t);
    __syncthreads();
    if (k + d < G) relem_combine_lds<NX>(e, sbuf + t + d, kSBS);
    __syncthreads();
  }
  // value function of node k+1, then ONE node-parallel Riccati step per lane: gains,
  // inertia test and (P_k, p_k) as the sequential recursion would produce them
  double Jn[NP + NX], nx_[NP + NX];
#pragma unroll
  for (int i = 0; i < NP; ++i) Jn[i] = e.J[i];
#pragma unroll
  for (int i = 0; i < NX; ++i) Jn[NP + i] = e.p[i];
  group_next<G, NP + NX>(Jn, nx_, xw);
  terminal_value<NX>(k, N, sgv, delta, gp, P, p);
  // (fmax returns its other operand for a NaN, so dev alone never sees one: the differences' sum
  // `tot` is finite only if every value is)
  double dev = 0.0, mag = 1.0, tot = 0.0;
  if (hasU) {
    okl = riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, false, AOneOf<Model>::value>(Hd, gp, Aop, Bop, cdef, nx_,
                                                                                           nx_ + NP, P, p, fac);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const double di = fabs(P[i] - e.J[i]);
      dev = fmax(dev, di);
      tot += di;
      mag = fmax(mag, fabs(P[i]));
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double di = fabs(p[i] - e.p[i]);
      dev = fmax(dev, di);
      tot += di;
      mag = fmax(mag, fabs(p[i]));
    }
  }
  // scan usable: stage R positive definite, finite, and consistent with the step
  const bool good = eok && dev <= 1e-8 * mag && tot < INFINITY;  // (tot: false for NaN and Inf)
  return !gall<G, G * R>(good, xw);
}

// ---- decoupled suffix (linear models; riccati.h DEC): what the sequential chains share.  With
// P_{k+1} reused, s = P_{k+1} c + p_{k+1} needs only p on the chain; P_{k+1} c (vpc) comes from the
// stored Pk of node k+1, off the chain.
template <class Model>
struct DecSuffix {
  bool reuse = false;  // group-uniform: this factorisation reuses the stored suffix (delta = 0)
  int kb = 0;          // first stage of the decoupled suffix
  int jc = 0;          // steps j >= jc are reused-suffix steps for every group of the wave (N: none)
  bool okd = true;     // this lane's verdict of its reused stage's factors
  double vpc[DecSuffixOf<Model>::value ? Model::NX : 1];
};
// vpc on every lane; on the reused stages the factors and P_k, set here, off the chain (dec_prefactor)
template <class Model, int G>
__device__ __forceinline__ void dec_suffix_setup(int k, int N, const double* Hd, const double* cdef, const double* Pk,
                                                 XWave<G>& xw, DecSuffix<Model>& ds, double* P,
                                                 Fac<Model::NX, Model::NU>& fac) {
  constexpr int NX = Model::NX, NU = Model::NU, NP = NX * (NX + 1) / 2;
  double Pn1[NP];
  group_next<G, NP>(Pk, Pn1, xw);
#pragma unroll
  for (int i = 0; i < NX; ++i) ds.vpc[i] = riccati_pc_row<NX>(Pn1, cdef, i);
  if (ds.reuse && k >= ds.kb && k < N) {
    ds.okd = dec_prefactor<NX, NU>(Hd, fac);
#pragma unroll
    for (int i = 0; i < NP; ++i) P[i] = Pk[i];
  }
}
// jc: steps j >= jc are reused-suffix steps for every group of the wave: they run first, in
// a loop of their own that moves only p (the same operations as the mixed loop's cheap
// steps; A stays in the stage table: 25 more live registers here measured slower)
template <int G>
__device__ __forceinline__ int dec_suffix_split(bool reuse, int kb, int N) {
  int jc = N;
  if (__all(reuse)) {
    XWave<64> xw1{nullptr, 0};
    jc = G >= 64 ? kb : (int)greduce<64, OpMax>((double)kb, xw1);  // max over the wave's groups
    jc = __builtin_amdgcn_readfirstlane(jc);  // wave-uniform: scalar loop bounds
  }
  return jc;
}

// The reused suffix as a log-depth scan (multi-wave groups: one instance per block).  On
// a reused stage p_k = A^T p_{k+1} + r_k with r_k = gp_x + A^T (P_{k+1} c), and when every
// stage of the suffix uses the same table (shared tables) the composition of d steps is
// the uniform (A^T)^d: a radix-4 Hillis-Steele suffix scan
//   v_k += (A^T)^d v_{k+d} + (A^T)^{2d} v_{k+2d} + (A^T)^{3d} v_{k+3d},   d = 1, 4, 16, 64
// carries only the NX-vector through ping-pong LDS buffers, ONE barrier per level (config 5:
// 4 levels replace the suffix's 95 dependent steps; a radix-2 scan needs 7 levels of two
// barriers).  The powers (A^T)^(j 4^l) depend only on the table: they are formed by NX^2
// threads in LDS the first time a launch scans a table and kept there for the launch.
// `Atab`: the shared stage tables' A (table i at Atab + i NX^2), `Amine`: this lane's stage table;
// `shared_tables`: one schedule for the batch and the launch; `dscan`: two NX-double buffers per
// thread, then the 15 powers; `pow_tab`: the table whose powers dscan holds (block-uniform).
// Returns true (group-uniform) when the scan ran: the suffix's p_k and factors are then set.
template <class Model, int G>
__device__ __forceinline__ bool suffix_scan(int k, int N, bool seq, const DecSuffix<Model>& ds, bool shared_tables,
                                            const double* Atab, const double* Amine, const double* gp,
                                            const double* Aop, double* dscan, double& pow_tab, XWave<G>& xw, double* p,
                                            Fac<Model::NX, Model::NU>& fac, bool& okl) {
  constexpr int NX = Model::NX, NU = Model::NU;
  constexpr int kSBS = G > 64 ? G : 64;
  const int jc = ds.jc;
  bool sscan = false;  // group-uniform
  if (jc < N && shared_tables) {
    const bool mine = k >= jc && k < N;
    const double ti = (double)((Amine - Atab) / (NX * NX));  // my stage's table
    double tt[2] = {mine ? ti : -1.0, mine ? ti : 1e300};
    greduce_n<G, 1, 2>(tt, xw);
    const double tmax = tt[0];
    sscan = tt[1] == tmax;
    if (sscan) {
      double* mpow = dscan + 2 * NX * kSBS;  // (A^T)^(j 4^l) at mpow[(3 l + j - 1) NX^2], row-major
      const int t = (int)threadIdx.x;
      constexpr int kLev = G > 64 ? (G <= 256 ? 4 : 5) : 1;  // 4^kLev >= G
      if (tmax != pow_tab) {  // block-uniform
        const double* Au = Atab + (size_t)tmax * NX * NX;
        auto mul = [&](int dst, int x, int y) __attribute__((always_inline)) {  // mpow[dst] = X Y
          if (t < NX * NX) {
            const double* X = mpow + x * NX * NX;
            const double* Y = mpow + y * NX * NX;
            const int i = t / NX, j = t % NX;
            double acc = X[i * NX] * Y[j];
#pragma unroll
            for (int m = 1; m < NX; ++m) acc = fma(X[i * NX + m], Y[m * NX + j], acc);
            mpow[dst * NX * NX + t] = acc;
          }
          __syncthreads();
        };
        if (t < NX * NX) mpow[t] = Au[(t % NX) * NX + t / NX];
        __syncthreads();
        for (int l = 0; l < kLev; ++l) {
          if (l > 0) mul(3 * l, 3 * l - 2, 3 * l - 2);  // (A^T)^(4^l) = ((A^T)^(2 4^(l-1)))^2
          mul(3 * l + 1, 3 * l, 3 * l);                 // (A^T)^(2 4^l)
          mul(3 * l + 2, 3 * l + 1, 3 * l);             // (A^T)^(3 4^l)
        }
        pow_tab = tmax;
      }
      double v[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        double acc = gp[i];
#pragma unroll
        for (int m = 0; m < NX; ++m)
          if (Model::AMASK & (1ull << (m * NX + i))) acc = fma(Aop[m * NX + i], ds.vpc[m], acc);
        v[i] = mine ? acc : (k == N ? p[i] : 0.0);
      }
      double* buf = dscan;  // ping-pong: level l reads buf[l % 2], writes buf[(l + 1) % 2]
#pragma unroll
      for (int i = 0; i < NX; ++i) buf[i * kSBS + t] = v[i];
      __syncthreads();
      for (int l = 0, d = 1; l < kLev && d <= N; ++l, d *= 4) {
        const double* cur = dscan + (l & 1) * NX * kSBS;
        double* nxt = dscan + ((l + 1) & 1) * NX * kSBS;
#pragma unroll
        for (int q = 1; q <= 3; ++q) {
          // the matrix spread over each 16-lane row (lane r: elements r and 16 + r) and
          // applied by row-broadcast FMAs (collectives.h matvec_bcast): the block-uniform
          // elements were 25 broadcast LDS reads, each a round trip on the FMA chain.  Every
          // lane takes part (a broadcast source lane must be active); lanes without a
          // partner keep v.
          const double* M = mpow + (3 * l + q - 1) * NX * NX;
          const int r = t & 15;
          const double mA = M[min(r, NX * NX - 1)];  // (in bounds for NX * NX < 16 too)
          const double mB = NX * NX > 16 ? M[16 + min(r, NX * NX - 17)] : 0.0;
          const bool on = t + q * d < G;
          const int src = on ? t + q * d : t;
          double w[NX], acc[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            w[i] = cur[i * kSBS + src];
            acc[i] = v[i];
          }
          matvec_bcast<NX>(acc, w, mA, mB);
#pragma unroll
          for (int i = 0; i < NX; ++i) v[i] = on ? acc[i] : v[i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) nxt[i * kSBS + t] = v[i];
        __syncthreads();
      }
      if (seq && mine) {
#pragma unroll
        for (int i = 0; i < NX; ++i) p[i] = v[i];
        fac.g0 = gp[NX];
        if constexpr (NU == 2) fac.g1 = fma(-fac.t, gp[NX], gp[NX + 1]);
        okl = ds.okd;
      }
    }
  }
  return sscan;
}

// ---- the row chain (rowchain.h): the node lanes hand their stages to LDS records, every row runs
// its instance's whole recursion, and node lane k takes step k's results back -- the same
// operations as riccati_step, so the same bits.  `rcbuf`: G records per instance of the wave;
// `Hsrc`: the stage Hessian without Sigma and delta (Hd = Hsrc + diag(sgv + delta)); `terminal(Pt,
// pt)`: node N's value function on its lane, zeros elsewhere (the kernel's: terminal_value).
template <class Model, int G, int R, class Terminal>
__device__ __forceinline__ void backward_rowchain(int k, int N, bool hasU, bool hasX, bool seq, int rho,
                                                  const double* Hd, const double* Hsrc, const double* sgv, double delta,
                                                  const double* gp, const double* Aop, const double* Bop,
                                                  const double* cdef, Terminal&& terminal, double* rcbuf, double* P,
                                                  double* p, Fac<Model::NX, Model::NU>& fac,
                                                  bool& okl MPCX_STAMP_PARAMS) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  static_assert(!DecSuffixOf<Model>::value && !WsStashOf<Model>::value, "row chain: plain sequential recursion only");
  int rslot = (int)((threadIdx.x & 63) / (G * R)) * G * rowchain::kRec;
  asm volatile("" : "+v"(rslot));  // (not hoisted out of the solve loop: one register less there)
  double* rinst = rcbuf + rslot;
  if (seq && (R == 1 || rho == 0)) {
    if (hasU) {
      rowchain::store_stage(rinst + k * rowchain::kRec, Hd, gp, Aop, Bop, cdef);
    } else if (hasX && k == N) {
      double PN[NP], pN[NX];
      terminal(PN, pN);
      rowchain::store_terminal(rinst + k * rowchain::kRec, PN, pN);
    }
  }
  // one wave per workgroup (G R <= 64): its LDS accesses complete in issue order, so the
  // hand-overs need only a compiler barrier, no s_barrier and no wait for the stores
  static_assert(G * R <= 64, "row chain: single-wave workgroups");
  asm volatile("" ::: "memory");
  STAMP_SUB(11);  // (diagnostic build: the chain itself as sub-phase 11, unused by this model)
  rowchain::run<G * R>(rinst, N);
  asm volatile("" ::: "memory");
  STAMP_SUB(12);
  // every node redoes its own step from node k+1's value function -- the chain's step k, the
  // same function on the same operands -- for its factors and P_k, all nodes at once.  P, p and
  // the factors are (re)set only here, so none of them is live across the chain (node N and
  // the lanes past it: P_N / zeros and no factors, as the sequential recursion leaves them),
  // and the stage Hessian is formed again from its parts (the delta barrier keeps the compiler
  // from holding the pre-chain copy across the chain instead)
  if (seq) {
    if (hasU) {
      double Pin_[NP], pin_[NX], Hk[NH];
      rowchain::load_next(rinst + (k + 1) * rowchain::kRec, Pin_, pin_);
      double dlt = delta;
      asm volatile("" : "+v"(dlt));
#pragma unroll
      for (int i = 0; i < NH; ++i) Hk[i] = Hsrc[i];
#pragma unroll
      for (int i = 0; i < NZ; ++i) Hk[symix(i, i, NZ)] += sgv[i] + dlt;
      (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, false, AOneOf<Model>::value>(
          Hk, gp, Aop, Bop, cdef, Pin_, pin_, P, p, fac);
    } else {
      terminal(P, p);
      fac = Fac<NX, NU>{};
    }
    okl = !hasU || fac_ok<NX, NU>(fac);
  }
}

// ---- the 6-state row chain (rowchain6.h): the node lanes write their stages (from the
// workspace stash) into the LDS ring window by window, every row runs the instance's
// recursion and stores each node's value function into that node's workspace slots, and
// node lane k redoes its own step from node k+1's -- the chain's step k, the same
// operations as riccati_step, so the same bits -- for its factors and P_k.
// Node lane k's own step from node k+1's value function in the workspace:
template <class Model>
__device__ __forceinline__ void rowchain6_node_step(double* ws, long ws_stride, long gid, double delta, const double* gp,
                                                    const double* cdef, double* P, double* p,
                                                    Fac<Model::NX, Model::NU>& fac) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  constexpr ChainRec rec(NX, NU);
  double Pin_[NP], pin_[NX], Hj[NH], Aj[NX * NX], Bj[NX * NU];
  rowchain6::load_next(chain_record<Model>(ws, ws_stride, gid) + rec.size + rec.P, Pin_, pin_);
  chain_record_jac<Model>(chain_record<Model>(ws, ws_stride, gid), Aj, Bj);
  stage_hessian_ws<Model>(chain_record<Model>(ws, ws_stride, gid), delta, Hj);
  (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, false, AOneOf<Model>::value>(Hj, gp, Aj, Bj, cdef, Pin_,
                                                                                         pin_, P, p, fac);
}
// `ws`, `ws_stride`, `gid`: the workspace and this thread (chain_record; k = this thread's node, so
// node 0's record is thread gid - k's); `ring`: rowchain6::kRing doubles of LDS.  Returns true
// when the chain stopped early at a step failing the inertia test (okl = false then).
template <class Model>
__device__ __forceinline__ bool backward_rowchain6(int k, int N, bool hasU, bool hasX, bool valid, bool seq, double* ws,
                                                   long ws_stride, long gid, const double* sgv, double delta,
                                                   const double* gp, const double* cdef, double* ring, double* P,
                                                   double* p, Fac<Model::NX, Model::NU>& fac,
                                                   bool& okl MPCX_STAMP_PARAMS) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2;
  constexpr ChainRec rec(NX, NU);
  static_assert(!DecSuffixOf<Model>::value && WsStashOf<Model>::value,
                "6-state row chain: plain sequential recursion, workspace stash");
  auto fill = [&](int lo, int hi, bool top) __attribute__((always_inline)) {
    if (seq && hasU && k >= lo && k <= hi) {
      const double* r = chain_record<Model>(ws, ws_stride, gid);
      double Hs_[NH], sg_[NZ], A_[NX * NX], B_[NX * NU];
#pragma unroll
      for (int i = 0; i < NH; ++i) Hs_[i] = wsload(r, rec.H + i);
#pragma unroll
      for (int i = 0; i < NZ; ++i) sg_[i] = wsload(r, rec.S + i);
      chain_record_jac<Model>(chain_record<Model>(ws, ws_stride, gid), A_, B_);
      rowchain6::store_node(ring + (k - lo) * rowchain6::kRec, Hs_, sg_, delta, A_, B_, gp, cdef);
    }
    if (top && seq && hasX && k == N) rowchain6::store_terminal(ring + (N - lo) * rowchain6::kRec, sgv, delta, gp);
  };
  double* out0 = ws + (long)RestoWs::slots(NX, NU) * ws_stride + (gid - k) * rec.size + rec.P;  // node 0's slots
  STAMP_SUB(11);
  const bool early = rowchain6::run(ring, out0, rec.size, valid && seq, N, fill);
  __syncthreads();  // row 0's workspace stores, before the node lanes read them
  STAMP_SUB(12);
  if (early) {
    // a step's reduced Huu' failed the inertia test (the chain stopped there): the attempt
    // fails whatever the other steps give -- the same decision as fac_ok after the full chain
    okl = false;
  } else if (seq) {
    if (hasU) {
      rowchain6_node_step<Model>(ws, ws_stride, gid, delta, gp, cdef, P, p, fac);
    } else {
      terminal_value<NX>(k, N, sgv, delta, gp, P, p);
      fac = Fac<NX, NU>{};
    }
    okl = !hasU || fac_ok<NX, NU>(fac);
  }
  return early;
}

// ---- the sequential chain of a single-wave group (G <= 64): one step per node, lane j only, the
// value function moved lane to lane by DPP.  P, p come in holding node N's value function
// (terminal_value) and, on a reused decoupled suffix, the stored P_k (dec_suffix_setup).  The
// operands of step j: registers (Hd, Aop, Bop), or -- models with a workspace chain stash -- lane
// j's record (ws, ws_stride, gid: chain_record).
template <class Model, int G>
__device__ __forceinline__ void backward_chain(int k, int N, bool hasU, bool seq, const DecSuffix<Model>& ds,
                                               const double* Hd, double delta, const double* gp, const double* Aop,
                                               const double* Bop, const double* cdef, double* ws, long ws_stride,
                                               long gid, double* P, double* p, Fac<Model::NX, Model::NU>& fac,
                                               bool& okl) {
  constexpr int NX = Model::NX, NU = Model::NU, NZ = NX + NU, NH = NZ * (NZ + 1) / 2, NP = NX * (NX + 1) / 2;
  constexpr bool kDec = DecSuffixOf<Model>::value, kWsStash = WsStashOf<Model>::value;
  const bool reuse = ds.reuse, okd = ds.okd;
  const int kb = ds.kb, jc = ds.jc;
  if constexpr (kDec) {
    for (int j = N - 1; j >= jc; --j) {
      double pin_[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
      if (seq && k == j) {
        dec_vector_step<NX, NU, Model::AMASK, Model::BMASK>(gp, Aop, Bop, ds.vpc, pin_, p, fac);
        okl = okd;
      }
    }
  }
  // models with a long chain step (the workspace-stash models, one instance per wave): a
  // failed inertia test ends the chain early (below)
  constexpr bool kEarly = kWsStash && !kDec && G == 64;
  bool early = false;
  // the chain: one step per node, lane j only.  Models without the decoupled suffix take
  // the inertia verdict of their step from its factors after the chain, on all lanes at
  // once (fac_ok), so no lane-mask merge sits on the chain
#pragma unroll 2
  for (int j = min(N, jc) - 1; j >= 0; --j) {
    const bool cheap = reuse && j >= kb;
    double Pin_[NP], pin_[NX];
    if (!kDec || __any(!cheap)) {
#pragma unroll
      for (int i = 0; i < NP; ++i) Pin_[i] = from_next(P[i]);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
    if (seq && k == j) {
      if constexpr (kDec) {
        if (cheap) {  // group-uniform
          dec_vector_step<NX, NU, Model::AMASK, Model::BMASK>(gp, Aop, Bop, ds.vpc, pin_, p, fac);
          okl = okd;
        } else {
          okl = riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, kDec, AOneOf<Model>::value>(
              Hd, gp, Aop, Bop, cdef, Pin_, pin_, P, p, fac);
        }
      } else if constexpr (kWsStash) {
        // this step's operands from the workspace (lane j only): no lane keeps its stage
        // Hessian and Jacobians in registers across the chain
        double Hj[NH], Aj[NX * NX], Bj[NX * NU];
        chain_record_jac<Model>(chain_record<Model>(ws, ws_stride, gid), Aj, Bj);
        stage_hessian_ws<Model>(chain_record<Model>(ws, ws_stride, gid), delta, Hj);
        (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, kDec, AOneOf<Model>::value>(
            Hj, gp, Aj, Bj, cdef, Pin_, pin_, P, p, fac);
      } else {
        (void)riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, kDec, AOneOf<Model>::value>(
            Hd, gp, Aop, Bop, cdef, Pin_, pin_, P, p, fac);
      }
    }
    // a step whose reduced Huu' is not positive definite decides the attempt: the KKT
    // matrix has the wrong inertia whatever the remaining steps give, so the chain stops
    // there (one instance per wave, so the verdict is the wave's).  Same decision, same
    // delta sequence as running the chain out (fac_ok is the test taken after the chain)
    if constexpr (kEarly) {
      if (__any(seq && k == j && !fac_ok<NX, NU>(fac))) {
        early = true;
        break;
      }
    }
  }
  if constexpr (!kDec)
    if (seq) okl = !early && (!hasU || fac_ok<NX, NU>(fac));
}

// ---- the sequential chain of a multi-wave group (G > 64, one workgroup per instance): wave by
// wave, N-side first; the value function crosses waves through the LDS exchange `xw`.  `sscan`:
// the suffix scan already ran the reused-suffix steps (suffix_scan).
template <class Model, int G>
__device__ __forceinline__ void backward_chain_waves(int k, int N, bool seq, const DecSuffix<Model>& ds, bool sscan,
                                                     const double* Hd, const double* gp, const double* Aop,
                                                     const double* Bop, const double* cdef, XWave<G>& xw, double* P,
                                                     double* p, Fac<Model::NX, Model::NU>& fac, bool& okl) {
  constexpr int NX = Model::NX, NU = Model::NU, NP = NX * (NX + 1) / 2;
  constexpr bool kDec = DecSuffixOf<Model>::value;
  const bool reuse = ds.reuse, okd = ds.okd;
  const int kb = ds.kb, jc = ds.jc;
  const int lane = threadIdx.x & 63;
  const int wv = (int)(threadIdx.x >> 6);
  for (int ph = XWave<G>::W - 1; ph >= 0; --ph) {
    if (wv == ph) {
      const double* in = xw.prev();  // (P, p) of node 64 (ph + 1), written last phase
      const int jtop = 64 * ph + 63;
      if constexpr (kDec) {  // this wave's reused-suffix steps (see dec_suffix_split)
        for (int j = min(N - 1, jtop); !sscan && j >= max(jc, 64 * ph); --j) {
          double pin_[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
          if (j == jtop && lane == 63)
#pragma unroll
            for (int i = 0; i < NX; ++i) pin_[i] = in[NP + i];
          if (seq && k == j) {
            dec_vector_step<NX, NU, Model::AMASK, Model::BMASK>(gp, Aop, Bop, ds.vpc, pin_, p, fac);
            okl = okd;
          }
        }
      }
      for (int j = min(min(N - 1, jtop), jc - 1); j >= 64 * ph; --j) {
        const bool cheap = reuse && j >= kb;
        double Pin_[NP], pin_[NX];
        if (!kDec || __any(!cheap)) {
#pragma unroll
          for (int i = 0; i < NP; ++i) Pin_[i] = from_next(P[i]);
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) pin_[i] = from_next(p[i]);
        if (j == jtop && lane == 63) {
#pragma unroll
          for (int i = 0; i < NP; ++i) Pin_[i] = in[i];
#pragma unroll
          for (int i = 0; i < NX; ++i) pin_[i] = in[NP + i];
        }
        if (seq && k == j) {
          if (cheap) {  // group-uniform
            dec_vector_step<NX, NU, Model::AMASK, Model::BMASK>(gp, Aop, Bop, ds.vpc, pin_, p, fac);
            okl = okd;
          }
          else
            okl = riccati_step<NX, NU, Model::AMASK, Model::BMASK, false, kDec, AOneOf<Model>::value>(Hd, gp, Aop, Bop, cdef, Pin_, pin_, P, p,
                                                                                 fac);
        }
      }
      if (ph > 0 && lane == 0) {
        double* out = xw.cur();
#pragma unroll
        for (int i = 0; i < NP; ++i) out[i] = P[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) out[NP + i] = p[i];
      }
    }
    xw.sync();
  }
}

}  // namespace mpcx
