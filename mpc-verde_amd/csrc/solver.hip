// solver.hip -- model registry of the fused solve (kernels.h, one translation unit per model:
// solve_<model>.hip) and the RK4+Jacobian sweep kernel over B x N unicycle intervals.
//
// Replaces, for B independent instances at once, the reference's
//   sol = solver(x0=w0, lbx, ubx, lbg, ubg, p)     Casadi/multiple_shooting_casadi.py:235-242
// (DESIGN.md §3), and the function + Jacobian evaluations IPOPT requests from CasADi (§4).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "mpcx.h"
#include "solver.h"
#include "unicycle.h"

namespace mpcx {

// ------------------------------------------------------------------------------
// RK4 + Jacobian sweep over B x N unicycle intervals, tiled structure of arrays.
// One thread per instance walks its N intervals: X_{k+1} loaded for interval k stays in
// registers as interval k+1's X_k and x_ref is loaded once, so HBM sees exactly the
// compulsory bytes (reads (N+1)*3 + 2N + 3 doubles, writes 24N doubles per instance;
// DESIGN.md §4).  Layout: 64-instance tiles, tile index inside each stage (tix below), so
// every wave's loads/stores of one stage are contiguous 512-B rows of one block -- the
// store pattern HBM absorbs fastest on this part (tools/hbm_probe.hip).
// ------------------------------------------------------------------------------
constexpr int kRec = 24;  // fields of the per-stage sweep record
__device__ __forceinline__ size_t tix(int stage, int F, int i, long b, long T) {
  return (((size_t)stage * T + (b >> 6)) * F + i) * 64 + (b & 63);
}
// record index of field PAIR j (fields 2j, 2j+1) in units of 16 B: inside a tile's 12 KB
// block of one stage, lane b%64 owns 16 contiguous bytes of each 1 KB pair row
__device__ __forceinline__ size_t jpix(int stage, int j, long b, long T) {
  return (((size_t)stage * T + (b >> 6)) * (kRec / 2) + j) * 64 + (b & 63);
}

__global__ __launch_bounds__(256) void rk4_sens_kernel(int B, int N, StageParams sp, const double* __restrict__ X,
                                                       const double* __restrict__ U, const double* __restrict__ XR,
                                                       double* __restrict__ J) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long T = ((long)B + 63) / 64;
  v2d* __restrict__ J2 = reinterpret_cast<v2d*>(J);
  double x[3], xr[3];
  const double ur[2] = {0.0, 0.0};
  const double lz[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x[i] = X[tix(0, 3, i, b, T)];
    xr[i] = XR[tix(0, 3, i, b, T)];
  }
  for (int k = 0; k < N; ++k) {
    double u[2], xn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xn[i] = X[tix(k + 1, 3, i, b, T)];
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = U[tix(k, 2, i, b, T)];
    double xf[3], q, A[9], Bm[6], g[5], H[15];
    uni_derivs<false>(sp, x, u, xr, ur, lz, 1.0, xf, q, A, Bm, g, H);
    // one 24-field record per stage: c(3) q(1) A(9) B(6) grad q(5), stored as 12 field
    // pairs of 16 B per lane (1 KB per wave-instruction, nontemporal) -- a wave's whole
    // output of a stage is one contiguous 12 KB block
    double r[kRec];
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = xf[i] - xn[i];
    r[3] = q;
#pragma unroll
    for (int i = 0; i < 9; ++i) r[4 + i] = A[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) r[13 + i] = Bm[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) r[19 + i] = g[i];
#pragma unroll
    for (int j = 0; j < kRec / 2; ++j) {
      const v2d v = {r[2 * j], r[2 * j + 1]};
      __builtin_nontemporal_store(v, &J2[jpix(k, j, b, T)]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = xn[i];
  }
}

hipError_t launch_rk4_sens(int B, int N, const StageParams& sp, const double* X, const double* U, const double* XR,
                           double* J, hipStream_t stream) {
  const long blocks = ((long)B + 255) / 256;
  hipLaunchKernelGGL(rk4_sens_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, B, N, sp, X, U, XR, J);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------
// Validation of device-resident bounds (mpcx_set_bounds_dev): the checks the host makes on a
// call's lbw / ubw (capi.cpp check_bounds_vec) and the state-bounded flag (state_bounded), over
// steps x rows x nw entries.  Grid-stride loop, one wave reduction, then one atomic per wave and
// result word; the first offender in array order is the smallest key.
// ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void check_bounds_kernel(const double* __restrict__ lbw,
                                                           const double* __restrict__ ubw, long n, int nw, int nx,
                                                           int nu, unsigned long long* res) {
  const long stride = (long)gridDim.x * blockDim.x;
  unsigned long long first = kBoundsOk;
  int xb = 0;
  for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const int i = (int)(j % nw);
    if (i < nx) continue;  // X_0 is pinned by g_0: its bounds are never read
    const double l = lbw[j], u = ubw[j];
    const int kind = (l != l || u != u || l > u) ? 1 : (l == u && l > -1e19) ? 2 : 0;
    const unsigned long long key = 4ull * (unsigned long long)j + (unsigned)kind;
    if (kind != 0 && key < first) first = key;
    const bool state = (i - nx) % (nx + nu) >= nu;  // z_k = (U_k, X_{k+1}): a state of node k + 1 >= 1
    xb |= (state && (l > -1e19 || u < 1e19)) ? 1 : 0;
  }
  for (int o = warpSize / 2; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(first, o);
    first = other < first ? other : first;
    xb |= __shfl_xor(xb, o);
  }
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (first != kBoundsOk) atomicMin(&res[0], first);
    if (xb) atomicOr(&res[1], 1ull);
  }
}

hipError_t launch_check_bounds(const double* lbw, const double* ubw, long n, int nw, int nx, int nu,
                               unsigned long long* res, hipStream_t stream) {
  long blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(check_bounds_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, lbw, ubw, n, nw, nx, nu, res);
  return hipGetLastError();
}

// ---- model registry: every stage model and its solve units (solve_<model>.hip) -------
extern const ModelOps ops_unicycle, ops_unicycle_xfree, ops_unicycle_scan, ops_linear4, ops_linear5, ops_linear4x2,
    ops_kin_bicycle, ops_dyn_bicycle, ops_cartpole, ops_path_bicycle;

// unicycle, the linear-model shapes the reference's QPs need (4x1 lateral / cart-pole, 5x1
// cart-pole with the previous input as a state; 4x2 for two-input models), and the BASELINE's nonlinear ODE variants
static const ModelInfo kModels[] = {
    // id, ODE model, (nx, nu) fixed by the model, solve units
    {MPCX_MODEL_UNICYCLE, false, true, {&ops_unicycle_scan, &ops_unicycle, &ops_unicycle_xfree}},
    {MPCX_MODEL_LINEAR, false, false, {&ops_linear4, &ops_linear5, &ops_linear4x2}},
    {MPCX_MODEL_KIN_BICYCLE, true, true, {&ops_kin_bicycle}},
    {MPCX_MODEL_DYN_BICYCLE, true, true, {&ops_dyn_bicycle}},
    {MPCX_MODEL_CARTPOLE, true, true, {&ops_cartpole}},
    {MPCX_MODEL_PATH_BICYCLE, true, true, {&ops_path_bicycle}},
};

const ModelInfo* model_info(int model) {
  for (const ModelInfo& m : kModels)
    if (m.id == model) return &m;
  return nullptr;
}

// horizons from which the unicycle's Riccati recursion runs as a log-depth scan (models.h
// UnicycleScanModel): ceil(log2(N+1)) = 5 combine levels cost about as much as 25 chain steps
constexpr int kUnicycleScanMinN = 25;
// diagnostic knob: MPCX_UNICYCLE_SCAN_MIN_N overrides it (A/B of the two instantiations).  Only
// a whole number in [1, 256] is taken (256: the scan never runs); anything else keeps the default.
static int unicycle_scan_min_n() {
  static const int n = [] {
    const char* e = getenv("MPCX_UNICYCLE_SCAN_MIN_N");
    if (!e || !*e) return kUnicycleScanMinN;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    return (*end == '\0' && v >= 1 && v <= 256) ? (int)v : kUnicycleScanMinN;
  }();
  return n;
}

const ModelOps* model_ops(const SolveArgs& a) {
  const ModelInfo* m = model_info(a.model);
  if (!m) return nullptr;
  if (m->id == MPCX_MODEL_UNICYCLE)  // the row's units: scan, state-bounded, free states
    return m->units[a.N >= unicycle_scan_min_n() ? 0 : a.xbnd ? 1 : 2];
  if (m->fixed_dims) return m->units[0];
  for (const ModelOps* u : m->units)
    if (u && u->nx == a.nx && u->nu == a.nu) return u;
  return nullptr;
}

}  // namespace mpcx

#ifdef MPCX_STAMPS
// diagnostic build: every model unit holds its own copy of the buffer pointers
static int diag_set(int (*mpcx::ModelOps::*setter)(void*), void* d_buf) {
  int r = 0;
  for (const mpcx::ModelInfo& m : mpcx::kModels)
    for (const mpcx::ModelOps* u : m.units)
      if (u) r |= (u->*setter)(d_buf);
  return r;
}
extern "C" int mpcx_diag_set_stamp_buffer(void* d_buf) { return diag_set(&mpcx::ModelOps::set_stamps, d_buf); }
extern "C" int mpcx_diag_set_counter_buffer(void* d_buf) { return diag_set(&mpcx::ModelOps::set_counters, d_buf); }
#endif
