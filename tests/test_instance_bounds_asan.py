"""Sanitizer run (CPU, host code only) of mpcx_set_bounds_dev's argument checking:
tests/asan/instance_bounds_validation.cpp, a stand-alone program linked with capi.cpp built under
AddressSanitizer and UndefinedBehaviorSanitizer (the object tests/asan/Makefile makes for
capi_validation.cpp) and with the device units' objects of mpc-verde_amd/build.  On a machine
without a GPU the program makes the null-handle calls only."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "tests", "asan")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host",
       "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer"]


def test_instance_bounds_validation_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "mpc-verde_amd")], check=True)
    subprocess.run(["make", "-s", "-C", ASAN, "capi_san.o"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(ROOT, "mpc-verde_amd", "build", "*.o")))
            if not o.endswith("capi.cpp.o")]
    assert any(o.endswith("solver.hip.o") for o in objs)  # (the validation kernel's unit)
    drv, exe = str(tmp_path / "instance_bounds_validation.o"), str(tmp_path / "instance_bounds_asan")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include")]
                   + SAN + ["-c", os.path.join(ASAN, "instance_bounds_validation.cpp"), "-o", drv], check=True)
    subprocess.run([HIPCC, "--offload-arch=gfx950", drv, os.path.join(ASAN, "capi_san.o")] + objs
                   + ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-o", exe], check=True)
    # with a device present the HIP / HSA runtimes keep allocations of their own until exit: those are
    # not the code under test (leaks of capi.cpp and of the program itself are still reported)
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\n")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", LSAN_OPTIONS=f"suppressions={supp}"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "instance bounds validation clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
