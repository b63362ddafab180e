// path_bicycle_validation.cpp -- host-only driver of the C ABI's argument checking for
// MPCX_MODEL_PATH_BICYCLE, built with AddressSanitizer + UndefinedBehaviorSanitizer on the host
// code and run by tests/test_path_bicycle_asan.py on a machine with or without a GPU (the
// companion of capi_validation.cpp, which walks the other models).  Everything here must be
// decided before a device is touched.  Exit status 0 = every check behaved.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mpcx.h"

static int failures = 0;
#define EXPECT(c)                                                          \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

int main() {
  mpcx_spec s;
  for (int N : {1, 20, 255}) {
    EXPECT(mpcx_default_spec(&s, MPCX_MODEL_PATH_BICYCLE, N) == 0);
    EXPECT(s.model == MPCX_MODEL_PATH_BICYCLE && s.nx == 4 && s.nu == 2 && s.N == N && s.M == 1);
    EXPECT(s.cost == MPCX_COST_NODE && s.param_layout == MPCX_P_X0_STAGEREF);
    EXPECT(s.par[0] == 3.5 && s.par[1] == 1.0 && s.par[3] == 10.0 / (N + 1));
    EXPECT(s.lbx[3] == -0.384 && s.ubx[3] == 0.384 && s.lbu[0] == -0.1225 && s.ubu[0] == 0.1225);
  }
  EXPECT(mpcx_default_spec(&s, 6, 20) < 0);  // 6 stays unassigned
  EXPECT(mpcx_default_spec(&s, 8, 20) < 0);
  auto refused = [&](void (*edit)(mpcx_spec&)) {
    mpcx_spec t;
    mpcx_default_spec(&t, MPCX_MODEL_PATH_BICYCLE, 20);
    edit(t);
    mpcx_handle* h = nullptr;
    const int r = mpcx_create(&t, &h);
    EXPECT(r == MPCX_EINVAL && h == nullptr);
    EXPECT(std::strlen(mpcx_last_error()) > 0);
  };
  refused([](mpcx_spec& t) { t.param_layout = MPCX_P_X0_XREF; });
  refused([](mpcx_spec& t) { t.cost = MPCX_COST_QUADRATURE; });
  refused([](mpcx_spec& t) { t.par[0] = 0.0; });
  refused([](mpcx_spec& t) { t.par[0] = -3.5; });
  refused([](mpcx_spec& t) { t.par[0] = NAN; });
  refused([](mpcx_spec& t) { t.par[1] = INFINITY; });
  refused([](mpcx_spec& t) { t.par[2] = NAN; });
  refused([](mpcx_spec& t) { t.par[3] = -INFINITY; });
  refused([](mpcx_spec& t) { t.lbx[3] = 0.5; t.ubx[3] = 0.384; });
  refused([](mpcx_spec& t) { t.lbu[0] = t.ubu[0]; });
  refused([](mpcx_spec& t) { t.T = 0.0; });
  refused([](mpcx_spec& t) { t.N = 0; });
  if (failures) {
    std::printf("FAILED (%d failures)\n", failures);
    return 1;
  }
  std::printf("path bicycle validation clean (0 failures)\n");
  return 0;
}
