// resto_check.hip -- test harness for the small dense routines of the restoration phase
// (mpc-verde_amd/csrc/resto.h): chol_small / chol_solve_small, resto_chol and resto_transform, for
// NX = 3, 4 and 6 (the state dimensions of the models that declare kResto).  One kernel per function,
// one thread per case; each kernel calls the very function recover() calls and writes its outputs and
// its verdict.  Built into tests/hip/libresto_check.so (tests/hip/Makefile); used by
// tests/test_gpu_resto_algebra.py only, which compares with the exact rational reference
// tests/helpers/resto_ref.py.
#include "kernels.h"

namespace mpcx {

// S: n x n (row-major, full), b: n  ->  out: L n x n, then x = S^-1 b (n)
template <int n>
__global__ void chol_check_kernel(int cases, const double* S, const double* b, double* out, int* ok) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cases) return;
  double s[n * n], L[n * n], x[n];
  for (int i = 0; i < n * n; ++i) s[i] = S[(size_t)c * n * n + i];
  for (int i = 0; i < n; ++i) x[i] = b[(size_t)c * n + i];
  ok[c] = chol_small<n>(s, L) ? 1 : 0;
  chol_solve_small<n>(L, x);
  double* o = out + (size_t)c * (n * n + n);
  for (int i = 0; i < n * n; ++i) o[i] = L[i];
  for (int i = 0; i < n; ++i) o[n * n + i] = x[i];
}

// D: NX, P: NP (packed, symix)  ->  out: Di NX, then L NX x NX
template <int NX>
__global__ void resto_chol_check_kernel(int cases, const double* D, const double* P, double* out, int* ok) {
  constexpr int NP = NX * (NX + 1) / 2;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cases) return;
  double d[NX], pk[NP], Di[NX], L[NX * NX];
  for (int i = 0; i < NX; ++i) d[i] = D[(size_t)c * NX + i];
  for (int i = 0; i < NP; ++i) pk[i] = P[(size_t)c * NP + i];
  ok[c] = resto_chol<NX>(d, pk, Di, L) ? 1 : 0;
  double* o = out + (size_t)c * (NX + NX * NX);
  for (int i = 0; i < NX; ++i) o[i] = Di[i];
  for (int i = 0; i < NX * NX; ++i) o[NX + i] = L[i];
}

// D: NX, P: NP (packed, symix), p: NX  ->  out: the transformed P (NP), then p (NX)
template <int NX>
__global__ void resto_transform_check_kernel(int cases, const double* D, const double* P, const double* p, double* out,
                                             int* ok) {
  constexpr int NP = NX * (NX + 1) / 2;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cases) return;
  double d[NX], pk[NP], pv[NX];
  for (int i = 0; i < NX; ++i) d[i] = D[(size_t)c * NX + i];
  for (int i = 0; i < NP; ++i) pk[i] = P[(size_t)c * NP + i];
  for (int i = 0; i < NX; ++i) pv[i] = p[(size_t)c * NX + i];
  ok[c] = resto_transform<NX>(d, pk, pv) ? 1 : 0;
  double* o = out + (size_t)c * (NP + NX);
  for (int i = 0; i < NP; ++i) o[i] = pk[i];
  for (int i = 0; i < NX; ++i) o[NP + i] = pv[i];
}

template <int NX>
int launch_resto_check(int which, int cases, const double* D, const double* M, const double* v, double* out, int* ok) {
  const dim3 grid((cases + 63) / 64), block(64);
  switch (which) {
    case 0: hipLaunchKernelGGL((chol_check_kernel<NX>), grid, block, 0, 0, cases, M, v, out, ok); break;
    case 1: hipLaunchKernelGGL((resto_chol_check_kernel<NX>), grid, block, 0, 0, cases, D, M, out, ok); break;
    case 2: hipLaunchKernelGGL((resto_transform_check_kernel<NX>), grid, block, 0, 0, cases, D, M, v, out, ok); break;
    default: return 1;
  }
  if (hipGetLastError() != hipSuccess) return 3;
  return hipDeviceSynchronize() == hipSuccess ? 0 : 3;
}

}  // namespace mpcx

// doubles written per case by function `which` at dimension nx; 0: no such function
extern "C" int resto_check_out_size(int which, int nx) {
  const int np = nx * (nx + 1) / 2;
  return which == 0 ? nx * nx + nx : which == 1 ? nx + nx * nx : which == 2 ? np + nx : 0;
}

// which: 0 chol_small + chol_solve_small (M = S, cases x nx x nx; v = b, cases x nx; D unused),
// 1 resto_chol (D cases x nx; M = P packed, cases x nx (nx + 1) / 2; v unused), 2 resto_transform (D, M = P
// packed, v = p).  out: cases x resto_check_out_size doubles, ok: cases ints; all device pointers.
// 1: bad argument, 2: no such instantiation, 3: the launch failed
extern "C" int resto_check(int which, int nx, int cases, const double* D, const double* M, const double* v, double* out,
                           int* ok) {
  using namespace mpcx;
  if (cases <= 0 || which < 0 || which > 2 || !M || !out || !ok) return 1;
  if ((which != 0 && !D) || (which != 1 && !v)) return 1;
  switch (nx) {
    case 3: return launch_resto_check<3>(which, cases, D, M, v, out, ok);
    case 4: return launch_resto_check<4>(which, cases, D, M, v, out, ok);
    case 6: return launch_resto_check<6>(which, cases, D, M, v, out, ok);
  }
  return 2;
}
