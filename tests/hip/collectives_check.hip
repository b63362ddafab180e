// collectives_check.hip -- test harness for the lane-group collectives of the solve kernels
// (mpc-verde_amd/csrc/collectives.h): every kernel calls the collectives the way the solve loop does
// and EVERY lane writes what it received, so the tests can compare the lanes of a group with each
// other.  Built into tests/hip/libcollectives_check.so (tests/hip/Makefile); used by
// tests/test_gpu_collectives.py only.
//
// Layout of the group kernels: inputs [cases][groups * G], outputs [cases][n_out][T] with
// T = blocks * block size lanes; the surplus lanes of the last block repeat the last group (as in
// filter_check.hip).  The loop over the cases has an argument-given bound, so every branch around
// an LDS exchange is block-uniform.
#include "collectives.h"

namespace mpcx {

constexpr int kReduceOut = 7;  // gsum gmax gmin | greduce_n<0, 1, 2, 3>
constexpr int kVoteOut = 4;    // gall gany | gall<G, 64> gany<G, 64> (G = 32 only, else the plain ones again)
constexpr int kMoveOut = 7;    // from_next from_prev | group_next<1> | group_next<3> | from_lane
constexpr int kScanOut = 3;    // prefix sum | prefix composition of affine maps (a, b)
constexpr int kDriftOut = 6;   // final value | slot after each of the five exchanges of round 0
constexpr int kElemOut = 3;    // qmax qmin qmax_abs

template <int G>
struct Lane {
  long gid, T;
  int k;
  long src;  // index of this lane's input inside one case
  __device__ Lane(int groups) {
    gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    T = (long)gridDim.x * blockDim.x;
    k = (int)(gid & (G - 1));
    const long g = gid / G;
    src = (g < groups ? g : groups - 1) * G + k;  // surplus lanes of the last block repeat a group
  }
};

template <int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void reduce_kernel(int groups, int cases, const double* v,
                                                                 const double* flag, double* out) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  XWave<G> xw{xch, 0};
  const Lane<G> l(groups);
  for (int c = 0; c < cases; ++c) {
    const double x = v[(long)c * groups * G + l.src], f = flag[(long)c * groups * G + l.src];
    double* o = out + (long)c * kReduceOut * l.T + l.gid;
    o[0 * l.T] = gsum<G>(x, xw);
    o[1 * l.T] = gmax<G>(x, xw);
    o[2 * l.T] = gmin<G>(x, xw);
    double t[4] = {x, x, x, f};
    greduce_n<G, 0, 1, 2, 3>(t, xw);
    for (int i = 0; i < 4; ++i) o[(3 + i) * l.T] = t[i];
  }
}

template <int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void vote_kernel(int groups, int cases, const int* cond, int* out) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  XWave<G> xw{xch, 0};
  const Lane<G> l(groups);
  for (int c = 0; c < cases; ++c) {
    const bool b = cond[(long)c * groups * G + l.src] != 0;
    int* o = out + (long)c * kVoteOut * l.T + l.gid;
    o[0 * l.T] = gall<G>(b, xw);
    o[1 * l.T] = gany<G>(b, xw);
    if constexpr (G == 32) {  // the replicated group of kernels.h (R = 2): the test is wave-wide
      o[2 * l.T] = gall<G, 64>(b, xw);
      o[3 * l.T] = gany<G, 64>(b, xw);
    } else {
      o[2 * l.T] = gall<G, G>(b, xw);
      o[3 * l.T] = gany<G, G>(b, xw);
    }
  }
}

template <int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void move_kernel(int groups, int cases, const double* v, const int* lane,
                                                               double* out) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  XWave<G> xw{xch, 0};
  const Lane<G> l(groups);
  for (int c = 0; c < cases; ++c) {
    const double x = v[(long)c * groups * G + l.src];
    const int s = lane[(long)c * groups * G + l.src] & 63;
    double* o = out + (long)c * kMoveOut * l.T + l.gid;
    o[0 * l.T] = from_next(x);
    o[1 * l.T] = from_prev(x);
    double n1[1], n3[3];
    const double x3[3] = {x, -x, 2.0 * x};  // exact images of x: the three slots stay apart
    group_next<G, 1>(&x, n1, xw);
    group_next<G, 3>(x3, n3, xw);
    o[2 * l.T] = n1[0];
    for (int i = 0; i < 3; ++i) o[(3 + i) * l.T] = n3[i];
    o[6 * l.T] = from_lane(x, s);
  }
}

// wave-wide inclusive scans with scan_partner / scan_takes, combined as kernels.h and sens.h combine
// them: the lane's own (later) element after the partner's (earlier) one
__global__ __launch_bounds__(64) void scan_kernel(const double* a, const double* b, double* out) {
  const long gid = (long)blockIdx.x * 64 + threadIdx.x, T = (long)gridDim.x * 64;
  const int kw = threadIdx.x & 63;
  double s = a[gid], am = a[gid], cm = b[gid];
  auto level = [&](auto dc) __attribute__((always_inline)) {
    constexpr int d = decltype(dc)::value;
    const double so = scan_partner<d>(s), ao = scan_partner<d>(am), co = scan_partner<d>(cm);
    if (scan_takes<d>(kw)) {
      s = so + s;
      cm = fma(am, co, cm);  // (am, cm) o (ao, co): x -> am (ao x + co) + cm
      am = am * ao;
    }
  };
  level(std::integral_constant<int, 1>{});
  level(std::integral_constant<int, 2>{});
  level(std::integral_constant<int, 4>{});
  level(std::integral_constant<int, 8>{});
  level(std::integral_constant<int, 16>{});
  level(std::integral_constant<int, 32>{});
  out[gid] = s;
  out[T + gid] = am;
  out[2 * T + gid] = cm;
}

// Exchange slots under drift (multi-wave groups): `rounds` rounds of gsum, greduce_n, group_next<1>,
// group_next<3>, gall; before every exchange each wave runs a different number of dependent FMAs,
// fixed by the wave index, the round and the position only.  The next value of a lane is an integer
// function of everything it received, so one value read from a slot too early or too late changes
// the result.  tests/helpers/collectives_ref.py drift_ref is the same sequence in NumPy.
__device__ __forceinline__ double spin(double d, int n, double c1, double c2) {
  for (int i = 0; i < n; ++i) d = fma(d, c1, c2);
  return d;
}
template <int G>
__global__ __launch_bounds__(G > 64 ? G : 64) void drift_kernel(int groups, int rounds, int work, double c1, double c2,
                                                                const double* v, double* trace, double* out, double* sink) {
  __shared__ double xch[2 * XWave<G>::W * kXchStride];
  XWave<G> xw{xch, 0};
  const Lane<G> l(groups);
  const int wv = threadIdx.x >> 6;
  long x = (long)v[l.src];
  double d = (double)l.k;
  for (int r = 0; r < rounds; ++r) {
    const double xd = (double)x;
    auto lag = [&](int p) { d = spin(d, work * ((wv * 3 + r * 5 + p * 7) % 11), c1, c2); };
    auto mark = [&](int p) {
      if (r == 0) out[(1 + p) * l.T + l.gid] = (double)xw.slot;
    };
    lag(0);
    const long s = (long)gsum<G>(xd, xw);
    mark(0);
    lag(1);
    double t[4] = {xd, xd, xd, x != (r * 7) % 61 ? 1.0 : 0.0};
    greduce_n<G, 0, 1, 2, 3>(t, xw);
    mark(1);
    lag(2);
    double n1[1], n3[3];
    group_next<G, 1>(&xd, n1, xw);
    mark(2);
    lag(3);
    const double x3[3] = {xd + 1.0, 2.0 * xd, xd + (double)s};
    group_next<G, 3>(x3, n3, xw);
    mark(3);
    lag(4);
    const bool a = gall<G>(x != (r * 11 + 3) % 61, xw);
    mark(4);
    const long acc = 3 * x + s + 5 * (long)t[0] + 7 * (long)t[1] + 11 * (long)t[2] + 13 * (long)t[3] + 17 * (long)n1[0] +
                     19 * (long)n3[0] + 23 * (long)n3[1] + 29 * (long)n3[2] + (a ? 31 : 0) + l.k + r;
    x = acc % 61;
    if (trace) trace[(long)r * l.T + l.gid] = (double)x;
  }
  out[l.gid] = (double)x;
  sink[l.gid] = d;  // keeps the FMA chains alive
}

__global__ void elem_kernel(long n, const double* a, const double* b, double* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = qmax(a[i], b[i]);
  out[n + i] = qmin(a[i], b[i]);
  out[2 * n + i] = qmax_abs(a[i], b[i]);
}

__global__ void rcp_kernel(long n, const double* x, double* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rcp64(x[i]);
}

static int finish() {
  if (hipGetLastError() != hipSuccess) return -1;
  return hipDeviceSynchronize() == hipSuccess ? 0 : -2;
}
template <int G>
static dim3 grid(int groups) {
  const int bs = G > 64 ? G : 64;
  return dim3((unsigned)(((long)groups * G + bs - 1) / bs));
}
template <int G>
static int launch(int what, int groups, int cases, const void* a, void* b, void* out, void* aux, int work, double c1,
                  double c2) {
  const dim3 gr = grid<G>(groups), bl(G > 64 ? G : 64);
  switch (what) {
    case 0:
      hipLaunchKernelGGL((reduce_kernel<G>), gr, bl, 0, 0, groups, cases, (const double*)a, (const double*)b, (double*)out);
      break;
    case 1: hipLaunchKernelGGL((vote_kernel<G>), gr, bl, 0, 0, groups, cases, (const int*)a, (int*)out); break;
    case 2:
      hipLaunchKernelGGL((move_kernel<G>), gr, bl, 0, 0, groups, cases, (const double*)a, (const int*)b, (double*)out);
      break;
    case 3:
      if (G <= 64) return -3;  // the drift check is about the LDS exchange
      hipLaunchKernelGGL((drift_kernel<G>), gr, bl, 0, 0, groups, cases, work, c1, c2, (const double*)a, (double*)b, (double*)out,
                         (double*)aux);
      break;
    default: return -3;
  }
  return finish();
}

}  // namespace mpcx

// lanes the group kernels write per output row: whole blocks of max(G, 64) threads
extern "C" long collectives_check_lanes(int G, int groups) {
  const long bs = G > 64 ? G : 64;
  return ((long)groups * G + bs - 1) / bs * bs;
}
// outputs per case of kernel `what` (0 reduce, 1 vote, 2 move, 3 drift; 4 scan, 5 elem)
extern "C" int collectives_check_outputs(int what) {
  const int n[6] = {mpcx::kReduceOut, mpcx::kVoteOut, mpcx::kMoveOut, mpcx::kDriftOut, mpcx::kScanOut, mpcx::kElemOut};
  return what >= 0 && what < 6 ? n[what] : -1;
}

// Device pointers; returns 0 on success.  what = 0 reduce (a values, b 0/1 flags as doubles), 1 vote
// (a int conditions), 2 move (a values, b int source lanes), 3 drift (a start values, cases =
// rounds, b = [rounds][lanes] values after every round or null, aux = sink of `lanes` doubles; one
// case of outputs).  Inputs [cases][groups * G], outputs
// [cases][outputs][lanes].
extern "C" int collectives_check(int what, int G, int groups, int cases, const void* a, void* b, void* out,
                                 void* aux, int work, double c1, double c2) {
  if (groups <= 0 || cases <= 0 || work < 0) return -3;
  switch (G) {
    case 16: return mpcx::launch<16>(what, groups, cases, a, b, out, aux, work, c1, c2);
    case 32: return mpcx::launch<32>(what, groups, cases, a, b, out, aux, work, c1, c2);
    case 64: return mpcx::launch<64>(what, groups, cases, a, b, out, aux, work, c1, c2);
    case 128: return mpcx::launch<128>(what, groups, cases, a, b, out, aux, work, c1, c2);
    case 256: return mpcx::launch<256>(what, groups, cases, a, b, out, aux, work, c1, c2);
  }
  return -3;
}

// a, b [waves * 64] -> out [3][waves * 64]
extern "C" int collectives_check_scan(int waves, const double* a, const double* b, double* out) {
  if (waves <= 0) return -3;
  hipLaunchKernelGGL(mpcx::scan_kernel, dim3(waves), dim3(64), 0, 0, a, b, out);
  return mpcx::finish();
}
// a, b [n] -> out [3][n]: qmax, qmin, qmax_abs
extern "C" int collectives_check_elem(long n, const double* a, const double* b, double* out) {
  if (n <= 0) return -3;
  hipLaunchKernelGGL(mpcx::elem_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, a, b, out);
  return mpcx::finish();
}
// x [n] -> out [n]: rcp64
extern "C" int collectives_check_rcp(long n, const double* x, double* out) {
  if (n <= 0) return -3;
  hipLaunchKernelGGL(mpcx::rcp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, x, out);
  return mpcx::finish();
}
