"""The manifold mean of the exact-shape Msckf update stops on |mean_delta|^2 > MEAN_STOP_SQ (csrc/slk_math.hpp) where the reference
tests |mean_delta| > 1e-6 (Msckf.hpp:511): tests/cpp/mean_stop_threshold.cpp checks that the constant is the largest double whose
correctly rounded square root is <= 1e-6 (sqrt(T) <= 1e-6 < sqrt(nextafter(T, inf))) and that s > T equals sqrt(s) > 1e-6 on four
thousand doubles on either side of it, on 0, the denormals, infinity, the NaNs and 4 * 10^5 random doubles; and that the exp
series' domain tests on the upper dword (nonneg_hi_below) equal x < 0.25 and x < 4.0 for every x that is +0, positive, +inf or
a NaN.  The program is the HOST half of the header (the device compiler's host pass, no device code in the binary) and runs on
the CPU; the device side meets one, two and three passes in tests/test_gpu_mean_loop_trim.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def test_mean_stop_threshold_equals_the_rule_on_the_norm():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mean_stop_threshold")
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "mean_stop_threshold.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "mean stop threshold ok" in out.stdout
