"""The release plan of the exact-shape Msckf update (csrc/slk_math.hpp: fast_release_plan -- behind which steps of the first
factorisation wave 0 meets the other waves, and which wave evaluates which feature in which pass) for every k = 4 .. 8 and
every one of the (k + 1)^4 pose tuples: tests/cpp/release_plan.cpp checks that every feature is assigned exactly once, that no
feature starts behind a barrier earlier than its own step, that the mask bits are live steps with A < B < C <= NKS - 2, that
every wave counts the same number of barriers, that the plan is the single release at ksmax with the second-pass rule where the
staggered condition fails, and the tabulated plans of the shapes that matter.  The program is the HOST half of the header (the
device compiler's host pass, no device code in the binary) and runs on the CPU; the device half runs the same function on
every filter of tests/test_gpu_staggered_release.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def test_release_plan_for_every_pose_tuple():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "release_plan")
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "release_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "release plan ok" in out.stdout
