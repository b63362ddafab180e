// instance_bounds_validation.cpp -- stand-alone driver of mpcx_set_bounds_dev's argument checking,
// built with AddressSanitizer + UndefinedBehaviorSanitizer on the host code and run by
// tests/test_instance_bounds_asan.py on a machine with or without a GPU.  Without a device only the
// null-handle calls can be made; with one, a unicycle handle walks the refusals that are decided
// before the device is touched, the device-side validation and the revert.  Exit status 0 = every
// check behaved.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

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
  double dummy[1] = {0.0};
  // a null handle is refused whatever else is passed
  EXPECT(mpcx_set_bounds_dev(nullptr, nullptr, nullptr, 1, 1, nullptr) == MPCX_EINVAL);
  EXPECT(std::strstr(mpcx_last_error(), "null handle") != nullptr);
  EXPECT(mpcx_set_bounds_dev(nullptr, dummy, dummy, 1, 1, nullptr) == MPCX_EINVAL);
  EXPECT(mpcx_set_bounds_dev(nullptr, dummy, nullptr, 0, 0, nullptr) == MPCX_EINVAL);

  mpcx_spec s;
  EXPECT(mpcx_default_spec(&s, MPCX_MODEL_UNICYCLE, 10) == 0);
  mpcx_handle* h = nullptr;
  const int rc = mpcx_create(&s, &h);
  if (rc == 0 && h) {  // a device is present
    int32_t nw = 0;
    EXPECT(mpcx_dims(h, &nw, nullptr, nullptr) == 0 && nw == 3 + 5 * 10);
    const int rows = 3;
    std::vector<double> lb((size_t)rows * nw, -1e20), ub((size_t)rows * nw, 1e20);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < 10; ++k) {
        lb[(size_t)r * nw + 3 + 5 * k] = -0.5 - 0.1 * r;
        ub[(size_t)r * nw + 3 + 5 * k] = 0.5 + 0.1 * r;
      }
    double *dl = nullptr, *du = nullptr;
    EXPECT(hipMalloc(&dl, lb.size() * sizeof(double)) == hipSuccess);
    EXPECT(hipMalloc(&du, ub.size() * sizeof(double)) == hipSuccess);
    auto upload = [&]() {
      EXPECT(hipMemcpy(dl, lb.data(), lb.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
      EXPECT(hipMemcpy(du, ub.data(), ub.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
    };
    upload();
    // decided before the device is touched
    EXPECT(mpcx_set_bounds_dev(h, dl, nullptr, rows, 1, nullptr) == MPCX_EINVAL);
    EXPECT(mpcx_set_bounds_dev(h, nullptr, du, rows, 1, nullptr) == MPCX_EINVAL);
    EXPECT(mpcx_set_bounds_dev(h, dl, du, 0, 1, nullptr) == MPCX_EINVAL);
    EXPECT(mpcx_set_bounds_dev(h, dl, du, -2, 1, nullptr) == MPCX_EINVAL);
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 0, nullptr) == MPCX_EINVAL);
    EXPECT(std::strlen(mpcx_last_error()) > 0);
    // accepted: per-instance rows, the same array as one shared row, as three steps of one row
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 1, nullptr) == 0);
    EXPECT(mpcx_set_bounds_dev(h, dl, du, 1, 1, nullptr) == 0);
    EXPECT(mpcx_set_bounds_dev(h, dl, du, 1, rows, nullptr) == 0);
    // refused by the device-side validation: the message names the entry
    lb[(size_t)1 * nw + 8] = 2.0;
    ub[(size_t)1 * nw + 8] = 1.0;
    upload();
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 1, nullptr) == MPCX_EINVAL);
    EXPECT(std::strstr(mpcx_last_error(), "row 1, index 8") != nullptr);
    lb[(size_t)1 * nw + 8] = NAN;
    upload();
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 1, nullptr) == MPCX_EINVAL);
    lb[(size_t)1 * nw + 8] = ub[(size_t)1 * nw + 8] = 1.0;
    upload();
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 1, nullptr) == MPCX_EINVAL);
    EXPECT(std::strstr(mpcx_last_error(), "fixed variable") != nullptr);
    // X_0's entries are not looked at
    lb[(size_t)1 * nw + 8] = -1.0;
    lb[(size_t)2 * nw + 1] = ub[(size_t)2 * nw + 1] = 0.25;
    upload();
    EXPECT(mpcx_set_bounds_dev(h, dl, du, rows, 1, nullptr) == 0);
    EXPECT(mpcx_set_bounds_dev(h, nullptr, nullptr, 1, 1, nullptr) == 0);  // revert
    EXPECT(mpcx_set_bounds_dev(h, nullptr, nullptr, 0, 0, nullptr) == 0);
    mpcx_destroy(h);
    (void)hipFree(dl);
    (void)hipFree(du);
    std::printf("instance bounds validation: device walk done\n");
  } else {
    EXPECT(rc == MPCX_EHIP && h == nullptr);  // no device: nothing more can be called
    std::printf("instance bounds validation: no device, null-handle calls only\n");
  }
  if (failures) {
    std::printf("FAILED (%d failures)\n", failures);
    return 1;
  }
  std::printf("instance bounds validation clean (0 failures)\n");
  return 0;
}
