"""The pivot test of the one-wave factorisations (csrc/slk_math.hpp: pivot_rank_neg, which the tile variant of the panel step
calls with the halves of -d, and pivot_not_positive; integer arithmetic on the two halves of a double) equals !(d > 0.0) for
every bit pattern: tests/cpp/pivot_predicate.cpp compares them on the
zeros, the denormals, DBL_MIN, DBL_MAX, the infinities, quiet and signalling NaNs of both signs, the upper halves next to
every boundary and 10^6 random patterns.  The program is the HOST half of the header (the device compiler's host pass, no
device code in the binary: the device half writes the same sum as a scalar compare and an add with carry) and runs on the
CPU; the device half meets a negative pivot, a NaN and an exact zero in tests/test_gpu_factor_chain_trim.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def test_pivot_predicate_equals_not_greater_than_zero():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pivot_predicate")
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "pivot_predicate.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "pivot predicate ok" in out.stdout
